"""Op-level parity of the LLM decode-step kernels (csrc/llm.hip) through the C ABI against float64 references computed on the CPU from the
already rounded operands, element-wise (tests/_helpers.py): cv_decode_attention (row-major three-kernel form and the fused form on
fragment-tiled caches), cv_rope_append, cv_kv_retile, cv_rmsnorm_reduce, cv_skinny_gemm (every dispatch branch) and cv_pack_skinny.

Outputs are NaN-prefilled with slack columns and rows that must stay NaN; inputs the ABI says are not read hold NaN, except the KV caches of
cv_decode_attention past the context: the kernel's precondition is a FINITE cache (stale keys meet P == 0), so those hold +-1e4 of mixed sign
— a key that leaks in takes the row over.

Bounds:
  decode attention  H.attn_bound (derived in tests/test_attention_ops_gpu.py: the same arithmetic per 64-key tile) with merge =
                    DECODE_MERGE_C = 10 for the 8-wave log-sum-exp merge: per wave one exp2 (1 ulp, common to numerator and denominator of a
                    wave but not across waves: 2 x 1), one product (0.5) and an 8-term fp32 sum (8 x 0.5) on each side: 2 + 1 + 8 = 11 half-
                    ulps on the numerator and the denominator together ~ 10 x 2^-23 with the max term exact.  The fused form's RoPE uses a
                    table of exact quarter turns (cos, sin in {0, +-1}) so that the roped query, which never leaves the registers, is known
                    bit for bit; the realistic table is checked through what the kernel appends to the cache.
  RoPE              H.rope_bound: angle = the single fp32 product fl32(pos * inv_freq[d]) (or the table entry), the rest in float64; rule 2
                    with n = 2, rule 3 for sincosf with e32 from torch's fp32 evaluation, half an ulp of the 16-bit output.
  retile / appends / pack_skinny   rule 1, bit-exact.
  rmsnorm_reduce    slab sum: rule 2 with n = nslab + 1; normalised row: H.rmsnorm_ref64 (rule 2 through rsqrt over dim terms), evaluated
                    from the row sums the op itself stored.
  skinny GEMM       modes 0 / 1: rule 2 with n = K (+ bias, + residual), sabs = |A| |W|^T; mode 3 the same through ReLU (1-Lipschitz); mode 2
                    SiLU as test_gemm_modes_gpu.py treats it (ACT_LIPSCHITZ, rule 3) and the product with u; prologue / split RMSNorm: the
                    RMSNorm bound b_A of the operand carried through |W| plus rule 2.
The ``test_cpu_*`` functions (no gpu mark) evaluate the same operations in plain torch on the same inputs and assert the SAME reference and
bound objects as the GPU tests (shared ``_*_expect`` / ``_split_checks`` helpers): the tiled emulation for decode attention, torch fp32 for RoPE,
RMSNorm and every skinny form (modes 0 / 1 per ksplit slab, mode 3 with its 16-bit rounding, mode 2, prologue + GEMM with the operand rounded
to the 16-bit type, split-norm producer / ss_part / consumer).  The decode-attention emulation misses its bound when the context is one key
too long (a poisoned key) or one key too short (the new token, which most cases make heavy), and, in the "flat" long-context cases where no
key dominates, when one 64-key tile beyond 1024 keys is left out."""
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _helpers as H  # noqa: E402

gpu = pytest.mark.gpu
DTS = [torch.bfloat16, torch.float16]
DT_IDS = ["bf16", "f16"]
NAN = float("nan")
POISON = 1.0e4


def _poison(shape, g):
    return torch.where(torch.rand(shape, generator=g) < 0.5, -POISON, POISON)


# ============================================================================= 1. cv_decode_attention
def _edges(ctx_max):
    s = {0, 1, ctx_max - 1}
    for k in range(1, ctx_max // 64):
        s |= {64 * k - 1, 64 * k, 64 * k + 1}
    return sorted(s)


def _chunks16(v):
    v = list(v)
    while len(v) % 16:
        v.append(v[len(v) % 7])
    return [tuple(v[i:i + 16]) for i in range(0, len(v), 16)]


LIST_A = (0, 63, 64, 511, 1022, 1023, 1024, 1025, 1086, 1087, 1088, 1534, 1535, 1536, 2046, 2047)
LIST_FLAT = (1087, 1088, 1151, 1152, 1279, 1280, 1535, 1536, 1537, 1599, 1663, 1791, 1919, 1983, 2046, 2047)
# (id, ctx_max, Hq, Hkv, positions of the new token = keys already cached; the row then sees pos + 1 keys)
DA_CASES = [(f"ctx2048-g7-b16-edges{n}", 2048, 14, 2, p) for n, p in enumerate(_chunks16(_edges(2048)))]
DA_CASES += [
    ("ctx2048-g1-b16", 2048, 2, 2, LIST_A), ("ctx2048-g16-b16", 2048, 16, 1, LIST_A),
    ("ctx2048-g7-b1-1535", 2048, 14, 2, (1535,)), ("ctx2048-g16-b1-2047", 2048, 16, 1, (2047,)), ("ctx2048-g1-b1-1087", 2048, 2, 2, (1087,)),
    ("ctx704-g7-b16", 704, 14, 2, (0, 1, 62, 63, 64, 65, 127, 128, 191, 192, 511, 512, 513, 640, 702, 703)),
    ("ctx704-g16-b16", 704, 16, 1, (0, 1, 62, 63, 64, 65, 127, 128, 191, 192, 511, 512, 513, 640, 702, 703)),
    ("ctx704-g1-b1-703", 704, 4, 4, (703,)),
    ("ctx64-g7-b16", 64, 14, 2, (0, 1, 2, 3, 7, 8, 15, 16, 17, 31, 32, 33, 47, 61, 62, 63)),
    ("ctx64-g1-b1-63", 64, 1, 1, (63,)), ("ctx64-g16-b1-0", 64, 16, 1, (0,)),
    # flat: the new token's key is as random as the rest, so every 64-key tile carries about 64 / n of a row's weight
    ("ctx2048-g7-b16-flat", 2048, 14, 2, LIST_FLAT), ("ctx2048-g1-b16-flat", 2048, 2, 2, LIST_FLAT), ("ctx2048-g16-b1-flat-2047", 2048, 16, 1, (2047,)),
]
DA_BY_ID = {c[0]: c for c in DA_CASES}
DA_IDS = list(DA_BY_ID)


@functools.lru_cache(maxsize=2)
def _da_data(cid, dt):
    """q (B, Hq, 64), K / V (B, Hkv, ctx_max, 64) as ``dt``: real keys in [0, pos], +-1e4 behind them.  The new token's key (index pos) is 9 x
    the mean query of its group, so that it carries a large share of every head's softmax: losing it is visible at any context length.  The
    "flat" cases keep a random key there instead: no key dominates, and a dropped or misplaced 64-key tile of a long context is what moves the
    output."""
    _, ctx_max, Hq, Hkv, pos = DA_BY_ID[cid]
    B, G = len(pos), Hq // Hkv
    g = torch.Generator().manual_seed(DA_IDS.index(cid) + 11)
    q = torch.randn(B, Hq, 64, generator=g).to(dt)
    k, v = torch.randn(B, Hkv, ctx_max, 64, generator=g), torch.randn(B, Hkv, ctx_max, 64, generator=g)
    kp, vp = _poison(k.shape, g), _poison(v.shape, g)
    knew = (9.0 * q.float().view(B, Hkv, G, 64).mean(2)).to(dt)
    for b, p in enumerate(pos):
        if "flat" not in cid:
            k[b, :, p] = knew[b].float()
        k[b, :, p + 1:], v[b, :, p + 1:] = kp[b, :, p + 1:], vp[b, :, p + 1:]
    return q, k.to(dt), v.to(dt)


def _da_mask(cid, d=0):
    _, ctx_max, _, _, pos = DA_BY_ID[cid]
    n = (torch.tensor(pos) + 1 + d).clamp(0, ctx_max)
    return (torch.arange(ctx_max)[None, :] < n[:, None])[:, None, :], n          # (B, 1, ctx_max)


@functools.lru_cache(maxsize=2)
def _da_ref(cid, dt):
    q, k, v = _da_data(cid, dt)
    ok, n = _da_mask(cid)
    kc, vc = torch.where(ok[:, :, :, None], k.double(), 0.0), torch.where(ok[:, :, :, None], v.double(), 0.0)   # the reference never touches the poison
    ref, A, S, sub = H.attn_ref64(q[:, :, None], kc, vc, 0.125, ok)
    bound = H.attn_bound(ref, A, S, sub, n.view(-1, 1, 1, 1), dt, merge=H.DECODE_MERGE_C)
    return ref[:, :, 0], bound[:, :, 0]


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("cid", DA_IDS)
def test_cpu_decode_attention_bound(cid, dt):
    """The torch emulation (64-key tiles dealt to 8 waves, merged by log-sum-exp) meets the bound on the inputs of every GPU case, and misses it
    with the context one key too long (the first poisoned key) or one key too short (the new token).  The flat cases have no heavy new
    token: there the emulation must miss the bound when one 64-key tile beyond key 1024 (keys 1024 .. 1087, the first tile of the reload
    loop) is left out, and one key too few is not asked of them (one flat key in two thousand is below the rounding of P in bf16)."""
    q, k, v = _da_data(cid, dt)
    ref, bound = _da_ref(cid, dt)
    ok, n = _da_mask(cid)
    H.check(f"emulated decode attention {cid}", H.attn_emulate(q[:, :, None], k, v, 0.125, ok, dt, waves=8)[:, :, 0], ref, bound)
    if dt == torch.float16:
        H.check(f"emulated decode attention {cid}, P flushed", H.attn_emulate(q[:, :, None], k, v, 0.125, ok, dt, waves=8, flush=True)[:, :, 0], ref, bound)
    if "flat" in cid:
        okd = ok.clone()
        okd[:, :, 1024:1088] = False
        got = H.attn_emulate(q[:, :, None], k, v, 0.125, okd, dt, waves=8)[:, :, 0].double()
        ratio = ((got - ref).abs() / bound.clamp_min(1e-300)).max().item()
        print(f"{cid}: tile 16 dropped -> max err/bound {ratio:.3g}")
        assert ratio > 1.0, f"{cid}: a dropped 64-key tile beyond 1024 keys stays inside the bound"
    for d in ((1,) if "flat" in cid else (1, -1)):
        okw, _ = _da_mask(cid, d)
        if torch.equal(okw, ok):
            continue
        got = H.attn_emulate(q[:, :, None], k, v, 0.125, okw, dt, waves=8)[:, :, 0].double()
        ratio = ((got - ref).abs() / bound.clamp_min(1e-300)).nan_to_num(float("inf")).max().item()
        print(f"{cid}: context {d:+d} -> max err/bound {ratio:.3g}")
        assert ratio > 1.0, f"{cid}: a context off by {d:+d} key stays inside the bound"


def _tile_cache(k, v):
    """Row-major (B, Hkv, ctx_max, 64) keys x d -> the two fragment-tiled caches (B, Hkv, ctx_max * 64), by the header's index map."""
    B, Hkv, ctx_max, _ = k.shape
    key, d = torch.meshgrid(torch.arange(ctx_max), torch.arange(64), indexing="ij")
    ik, iv = H.kv_tile_index(key, d).reshape(-1), H.kv_tile_index(key, d, v=True).reshape(-1)
    kt, vt = torch.empty(B, Hkv, ctx_max * 64, dtype=k.dtype), torch.empty(B, Hkv, ctx_max * 64, dtype=k.dtype)
    kt[..., ik] = k.reshape(B, Hkv, -1)
    vt[..., iv] = v.reshape(B, Hkv, -1)
    return kt, vt, ik.view(ctx_max, 64), iv.view(ctx_max, 64)


def _quarter_turn_table(ctx_max, g):
    """rope[ctx_max][64] = [cos 32 | sin 32] with every angle a multiple of 90 degrees: x1 c - x2 s is then exact in any type."""
    turn = torch.randint(0, 4, (ctx_max, 32), generator=g)
    c = torch.tensor([1.0, 0.0, -1.0, 0.0])[turn]
    s = torch.tensor([0.0, 1.0, 0.0, -1.0])[turn]
    return torch.cat([c, s], 1).contiguous()


def _unrope(x, tab_row):
    """The exact inverse of the quarter-turn RoPE: rotate by the negative angle."""
    c, s = tab_row[..., :32], tab_row[..., 32:]
    x1, x2 = x[..., :32], x[..., 32:]
    return torch.cat([x1 * c + x2 * s, x2 * c - x1 * s], -1)


@gpu
@pytest.mark.parametrize("form", ["rowmajor", "fused"])
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("cid", DA_IDS)
def test_decode_attention(cid, dt, form):
    """Contexts around every 64-key edge up to ctx_max, among them > 1024 keys (the loop that reloads a wave's tile pair: one tile per wave
    per round for 1025 .. 1536 keys, two beyond), Hq / Hkv 1, 7, 16, B 1 and 16, the new token in the last slot of a tile and of the cache."""
    from cosyvoice_amd import ops
    _, ctx_max, Hq, Hkv, pos = DA_BY_ID[cid]
    B, G = len(pos), Hq // Hkv
    q, k, v = _da_data(cid, dt)
    ref, bound = _da_ref(cid, dt)
    ldo = Hq * 64 + 4
    out = H.nan_like((B + 2, ldo), dt)
    ctx = torch.tensor(pos, dtype=torch.int32, device="cuda")
    if form == "rowmajor":
        qd = H.nan_like((B + 1, Hq * 64 + 8), dt)
        qd[:B, :Hq * 64] = q.reshape(B, Hq * 64).cuda()
        ops.decode_attention(qd, k.cuda(), v.transpose(2, 3).contiguous().cuda(), ctx, 1, out, B, Hq, Hkv, ctx_max, 0.125)
        torch.cuda.synchronize()
    else:
        g = torch.Generator().manual_seed(len(cid))
        tab = _quarter_turn_table(ctx_max, g)
        rows = tab[torch.tensor(pos)]                                           # (B, 64)
        width = (Hq + 2 * Hkv) * 64
        qkv = torch.full((B + 1, width + 4), NAN)
        knew, vnew = torch.stack([k[b, :, p] for b, p in enumerate(pos)]), torch.stack([v[b, :, p] for b, p in enumerate(pos)])   # (B, Hkv, 64)
        qkv[:B, :Hq * 64] = _unrope(q.float(), rows[:, None]).reshape(B, -1)
        qkv[:B, Hq * 64:(Hq + Hkv) * 64] = _unrope(knew.float(), rows[:, None]).reshape(B, -1)
        qkv[:B, (Hq + Hkv) * 64:width] = vnew.float().reshape(B, -1)
        k0, v0 = k.clone(), v.clone()
        pk, pv = _poison(knew.shape, g).to(dt), _poison(vnew.shape, g).to(dt)
        for b, p in enumerate(pos):                                               # the slot of the new token is stale before the call
            k0[b, :, p], v0[b, :, p] = pk[b], pv[b]
        kt0, vt0, ik, iv = _tile_cache(k0, v0)
        ktd, vtd = kt0.cuda(), vt0.cuda()
        ops.decode_attention(torch.empty(1, 8, dtype=dt, device="cuda"), ktd, vtd, ctx, 1, out, B, Hq, Hkv, ctx_max, 0.125, qkv=qkv.cuda(),
                             inv_freq=tab.cuda())
        torch.cuda.synchronize()
        kt1, vt1, _, _ = _tile_cache(k, v)                                       # what the caches must hold now: only position pos differs
        assert torch.equal(ktd.cpu().view(torch.int16), kt1.view(torch.int16)), "K cache: the roped new key at pos, nothing else changed"
        assert torch.equal(vtd.cpu().view(torch.int16), vt1.view(torch.int16)), "V^T cache: the new value at pos, nothing else changed"
    o = out.cpu().float()
    assert bool(torch.isnan(o[B:]).all()) and bool(torch.isnan(o[:, Hq * 64:]).all()), "decode attention wrote outside [B][Hq * 64]"
    res = o[:B, :Hq * 64].view(B, Hq, 64)
    H.check(f"decode_attention {form} {cid} [{dt}]", res, ref, bound)
    for b, p in enumerate(pos):
        if p == 0:                                                                # one key: softmax = 1, the output is the new token's V
            assert torch.equal(res[b].view(Hkv, G, 64), v[b, :, 0].float()[:, None].expand(Hkv, G, 64)), "ctx_len = 0: out must be V of the new token"


@gpu
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_decode_attention_empty_context_is_zero(dt):
    """ctx_len = 0 with ctx_add = 0 (three-kernel form): no key at all, the rows are exact zeros; the cache holds only poison."""
    from cosyvoice_amd import ops
    g = torch.Generator().manual_seed(3)
    B, Hq, Hkv, ctx_max = 3, 14, 2, 128
    q = torch.randn(B, Hq * 64, generator=g).to(dt).cuda()
    k, v = _poison((B, Hkv, ctx_max, 64), g).to(dt).cuda(), _poison((B, Hkv, 64, ctx_max), g).to(dt).cuda()
    out = H.nan_like((B + 2, Hq * 64 + 4), dt)
    ctx = torch.tensor([0, 5, 0], dtype=torch.int32, device="cuda")
    ops.decode_attention(q, k, v, ctx, 0, out, B, Hq, Hkv, ctx_max, 0.125)
    torch.cuda.synchronize()
    o = out.cpu().float()
    assert bool((o[[0, 2], :Hq * 64] == 0).all()), "no visible key: exact zeros"
    assert bool(torch.isfinite(o[1, :Hq * 64]).all())
    assert bool(torch.isnan(o[B:]).all()) and bool(torch.isnan(o[:, Hq * 64:]).all())


@gpu
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("ctx_max", [64, 704])
def test_decode_attention_fused_full_cache_is_left_alone(ctx_max, dt):
    """ctx_len >= ctx_max in the fused form: there is no slot for the new token; the caches stay bit-identical and the output is finite
    (include/cosyvoice_amd.h defines no more than that)."""
    from cosyvoice_amd import ops
    g = torch.Generator().manual_seed(ctx_max)
    B, Hq, Hkv = 4, 14, 2
    k, v = torch.randn(B, Hkv, ctx_max, 64, generator=g).to(dt), torch.randn(B, Hkv, ctx_max, 64, generator=g).to(dt)
    kt, vt, _, _ = _tile_cache(k, v)
    ktd, vtd = kt.cuda(), vt.cuda()
    ang = torch.arange(ctx_max, dtype=torch.float32)[:, None] * (1.0 / (1e6 ** (torch.arange(0, 64, 2, dtype=torch.float32) / 64)))[None]
    tab = torch.cat([ang.cos(), ang.sin()], 1).contiguous()
    qkv = torch.randn(B, (Hq + 2 * Hkv) * 64, generator=g)
    pos = [ctx_max, ctx_max + 1, ctx_max + 63, 5 * ctx_max]
    ctx = torch.tensor(pos, dtype=torch.int32, device="cuda")
    out = H.nan_like((B + 2, Hq * 64 + 4), dt)
    ops.decode_attention(torch.empty(1, 8, dtype=dt, device="cuda"), ktd, vtd, ctx, 1, out, B, Hq, Hkv, ctx_max, 0.125, qkv=qkv.cuda(),
                         inv_freq=tab.cuda())
    torch.cuda.synchronize()
    assert torch.equal(ktd.cpu().view(torch.int16), kt.view(torch.int16)) and torch.equal(vtd.cpu().view(torch.int16), vt.view(torch.int16))
    o = out.cpu().float()
    assert bool(torch.isfinite(o[:B, :Hq * 64]).all())
    assert bool(torch.isnan(o[B:]).all()) and bool(torch.isnan(o[:, Hq * 64:]).all())


INV_FREQ = 1.0 / (1e6 ** (torch.arange(0, 64, 2, dtype=torch.float32) / 64))


@gpu
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
def test_decode_attention_fused_rope_append(dt):
    """The fused form with the production cos / sin table and an fp32 qkv row: the key it appends is the float64 RoPE of the row with the
    table's fp32 cos / sin taken as given (no sincosf in this form: rule 2 with n = 2 + half an ulp), the value bit-exact, every other element
    of both caches unchanged."""
    from cosyvoice_amd import ops
    g = torch.Generator().manual_seed(17)
    B, Hq, Hkv, ctx_max = 16, 14, 2, 704
    pos = [0, 1, 31, 62, 63, 64, 65, 127, 128, 300, 511, 512, 639, 640, 702, 703]
    ang = torch.arange(ctx_max, dtype=torch.float32)[:, None] * INV_FREQ[None]
    tab = torch.cat([ang.cos(), ang.sin()], 1).contiguous()
    k, v = torch.randn(B, Hkv, ctx_max, 64, generator=g).to(dt), torch.randn(B, Hkv, ctx_max, 64, generator=g).to(dt)
    kt, vt, ik, iv = _tile_cache(k, v)
    ktd, vtd = kt.cuda(), vt.cuda()
    width = (Hq + 2 * Hkv) * 64
    qkv = torch.full((B + 1, width + 8), NAN)
    qkv[:B, :width] = torch.randn(B, width, generator=g) * 2
    out = H.nan_like((B + 2, Hq * 64 + 4), dt)
    ops.decode_attention(torch.empty(1, 8, dtype=dt, device="cuda"), ktd, vtd, torch.tensor(pos, dtype=torch.int32, device="cuda"), 1, out, B, Hq,
                         Hkv, ctx_max, 0.125, qkv=qkv.cuda(), inv_freq=tab.cuda())
    torch.cuda.synchronize()
    k1, v1 = ktd.cpu(), vtd.cpu()
    changed_k, changed_v = k1.view(torch.int16) != kt.view(torch.int16), v1.view(torch.int16) != vt.view(torch.int16)
    for b, p in enumerate(pos):
        may_k, may_v = torch.zeros(ctx_max * 64, dtype=torch.bool), torch.zeros(ctx_max * 64, dtype=torch.bool)
        may_k[ik[p]], may_v[iv[p]] = True, True
        assert not bool(changed_k[b][:, ~may_k].any()) and not bool(changed_v[b][:, ~may_v].any()), f"row {b}: wrote outside position {p}"
        kin = qkv[b, Hq * 64:(Hq + Hkv) * 64].view(Hkv, 64)
        ref, sabs = H.rope_table_ref64(kin, tab[p, :32], tab[p, 32:])
        H.check(f"fused append K pos {p} [{dt}]", k1[b][:, ik[p]], ref, H.sum_bound(2, sabs, ref, dt))
        assert torch.equal(v1[b][:, iv[p]], qkv[b, (Hq + Hkv) * 64:width].view(Hkv, 64).double().to(dt)), "appended V: bit-exact"
    o = out.cpu().float()
    assert bool(torch.isfinite(o[:B, :Hq * 64]).all())
    assert bool(torch.isnan(o[B:]).all()) and bool(torch.isnan(o[:, Hq * 64:]).all())


# ============================================================================= 2. cv_rope_append
ROPE_CASES = {
    "decode-rows1": (1, (0, 1, 63, 64, 500, 703, 704, 1023, 1024, 2046, 2047, 2048, 5000, 7, 2047, 100), 2048),
    "prefill-rows5": (5, (0, 59, 2043, 2046, 700), 2048),
    "prefill-rows282": (282, (0, 1700, 1900), 2048),
    "prefill-rows282-ctx704": (282, (0, 422, 423, 650), 704),
}


def _rope_case(name, dt):
    rps, base, ctx_max = ROPE_CASES[name]
    g = torch.Generator().manual_seed(len(name) + rps)
    B, Hq, Hkv = len(base), 14, 2
    rows, width = B * rps, (14 + 4) * 64
    qkv = torch.randn(rows, width, generator=g) * 2
    pos = (torch.tensor(base)[:, None] + torch.arange(rps)[None]).reshape(-1)                       # (rows,)
    ang = pos.float()[:, None] * INV_FREQ[None]                                                     # the single fp32 product
    xq, xk = qkv[:, :Hq * 64].view(rows, Hq, 64), qkv[:, Hq * 64:(Hq + Hkv) * 64].view(rows, Hkv, 64)
    q = H.rope_ref64(xq, ang[:, None].expand(rows, Hq, 32))
    k = H.rope_ref64(xk, ang[:, None].expand(rows, Hkv, 32))
    return qkv, pos, q, k, (B, Hq, Hkv, rps, ctx_max, rows, width)


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("name", list(ROPE_CASES))
def test_cpu_rope_bound_holds_for_torch_fp32(name, dt):
    _, _, (qr, qs, q32), (kr, ks, k32), _ = _rope_case(name, dt)
    H.check("torch fp32 rope q", q32.to(dt), qr, H.rope_bound(qr, qs, q32, dt))
    H.check("torch fp32 rope k", k32.to(dt), kr, H.rope_bound(kr, ks, k32, dt))


@gpu
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("name", list(ROPE_CASES))
def test_rope_append(name, dt):
    """rows_per_seq 1 (decode), 5 and 282 (prefill) with ragged pos_base, positions up to 2047 and beyond: rows at pos >= ctx_max write q_out
    only; the caches change at (b, h, pos) and nowhere else."""
    from cosyvoice_amd import ops
    qkv, pos, (qr, qs, q32), (kr, ks, k32), (B, Hq, Hkv, rps, ctx_max, rows, width) = _rope_case(name, dt)
    base = ROPE_CASES[name][1]
    ldqkv, ldq = width + 4, Hq * 64 + 8
    qin = H.nan_like((rows + 1, ldqkv), torch.float32)
    qin[:rows, :width] = qkv.cuda()
    qo = H.nan_like((rows + 2, ldq), dt)
    kc, vc = H.nan_like((B, Hkv, ctx_max, 64), dt), H.nan_like((B, Hkv, 64, ctx_max), dt)
    ops.rope_append(qin, torch.tensor(base, dtype=torch.int32, device="cuda"), rows, rps, Hq, Hkv, INV_FREQ.cuda(), qo, kc, vc, ctx_max)
    torch.cuda.synchronize()
    qo, kc, vc = qo.cpu(), kc.cpu(), vc.cpu()
    assert bool(torch.isnan(qo[rows:].float()).all()) and bool(torch.isnan(qo[:, Hq * 64:].float()).all()), "q_out guards"
    H.check(f"rope_append q {name} [{dt}]", qo[:rows, :Hq * 64].view(rows, Hq, 64), qr, H.rope_bound(qr, qs, q32, dt))
    bidx = torch.arange(rows) // rps
    inside = pos < ctx_max
    assert bool((~inside).any()) and bool(inside.any())
    written = torch.zeros(B, ctx_max, dtype=torch.bool)
    written[bidx[inside], pos[inside]] = True
    kb = H.rope_bound(kr, ks, k32, dt)
    H.check(f"rope_append K {name} [{dt}]", kc[bidx[inside], :, pos[inside]], kr[inside], kb[inside])
    vref = qkv[:, (Hq + Hkv) * 64:].view(rows, Hkv, 64).double().to(dt)
    assert torch.equal(vc[bidx[inside], :, :, pos[inside]], vref[inside]), "V^T column: bit-exact"
    assert bool(torch.isnan(kc.float()[~written[:, None].expand(B, Hkv, ctx_max)]).all()), "K cache rows that are nobody's position were written"
    assert bool(torch.isnan(vc.float().transpose(2, 3)[~written[:, None].expand(B, Hkv, ctx_max)]).all()), "V^T columns that are nobody's position were written"


# ============================================================================= 3. cv_kv_retile
@gpu
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("ctx_max", [64, 704])
@pytest.mark.parametrize("n_keys", [0, 1, 64, 65, "ctx_max"])
def test_kv_retile(n_keys, ctx_max, dt):
    """Every element against the documented index map; tiles at or past ceil(n_keys / 64) stay untouched."""
    from cosyvoice_amd import ops
    n_keys = min(ctx_max if n_keys == "ctx_max" else n_keys, ctx_max)
    g = torch.Generator().manual_seed(ctx_max + n_keys)
    B, Hkv = 3, 2
    k, v = torch.randn(B, Hkv, ctx_max, 64, generator=g).to(dt), torch.randn(B, Hkv, ctx_max, 64, generator=g).to(dt)
    ktd, vtd = H.nan_like((B, Hkv, ctx_max * 64), dt), H.nan_like((B, Hkv, ctx_max * 64), dt)
    ops.kv_retile(k.cuda(), v.transpose(2, 3).contiguous().cuda(), ktd, vtd, B, Hkv, ctx_max, n_keys)
    torch.cuda.synchronize()
    kt, vt, ik, iv = _tile_cache(k, v)
    nt = (n_keys + 63) // 64
    kd, vd = ktd.cpu(), vtd.cpu()
    assert torch.equal(kd[..., :nt * 4096], kt[..., :nt * 4096]) and torch.equal(vd[..., :nt * 4096], vt[..., :nt * 4096])
    assert bool(torch.isnan(kd[..., nt * 4096:].float()).all()) and bool(torch.isnan(vd[..., nt * 4096:].float()).all()), "tiles past n_keys were written"
    assert sorted(ik.reshape(-1).tolist()) == list(range(ctx_max * 64)) and sorted(iv.reshape(-1).tolist()) == list(range(ctx_max * 64))
    key, d = torch.meshgrid(torch.arange(ctx_max), torch.arange(64), indexing="ij")
    assert torch.equal(ops.kv_tile_index(ctx_max, key, d), ik) and torch.equal(ops.kv_tile_index(ctx_max, key, d, v=True), iv)


# ============================================================================= 4. cv_rmsnorm_reduce
def _rms_case(dim, rows, nslab):
    g = torch.Generator().manual_seed(dim + rows * 7 + nslab)
    x = torch.randn(rows, dim, generator=g)
    x[0] *= 1.0e4                                   # a large common scale
    if rows > 1:
        x[rows - 1] *= 1.0e-5                       # near zero: eps = 1e-6 dominates mean(x^2) = 1e-10
    slabs = torch.randn(max(nslab, 1), rows, dim, generator=g) * x.abs().mean(-1, keepdim=True)[None]
    gamma = torch.randn(dim, generator=g)
    return x, slabs, gamma


RMS_SHAPES = [(4, 1), (64, 3), (896, 3), (896, 16), (1024, 33), (1028, 3), (4096, 1), (4096, 16)]


@pytest.mark.parametrize("nslab", [0, 1, 2, 4])
@pytest.mark.parametrize("dim,rows", RMS_SHAPES)
def test_cpu_rmsnorm_bound_holds_for_torch_fp32(dim, rows, nslab):
    x, slabs, gamma = _rms_case(dim, rows, nslab)
    xs = x.clone()
    for s in range(nslab):
        xs = xs + slabs[s]
    ref = x.double() + slabs[:nslab].double().sum(0)
    H.check("torch fp32 slab sum", xs, ref, H.sum_bound(nslab + 1, x.double().abs() + slabs[:nslab].double().abs().sum(0), ref, torch.float32))
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        r, b = H.rmsnorm_ref64(xs, gamma, 1e-6, dt)
        t32 = xs * torch.rsqrt((xs * xs).mean(-1, keepdim=True) + 1e-6) * gamma
        H.check(f"torch fp32 rmsnorm [{dt}]", t32.to(dt), r, b)


@gpu
@pytest.mark.parametrize("dt", [torch.float32] + DTS, ids=["f32"] + DT_IDS)
@pytest.mark.parametrize("nslab", [0, 1, 2, 4])
@pytest.mark.parametrize("dim,rows", RMS_SHAPES)
def test_rmsnorm_reduce(dim, rows, nslab, dt):
    from cosyvoice_amd import ops
    x, slabs, gamma = _rms_case(dim, rows, nslab)
    ldx, ldxn, ld_slab = dim + 4, dim + 8, dim + 12
    xd = H.nan_like((rows + 2, ldx), torch.float32)
    xd[:rows, :dim] = x.cuda()
    sd = H.nan_like((max(nslab, 1), rows + 1, ld_slab), torch.float32)
    sd[:, :rows, :dim] = slabs.cuda()
    xn = H.nan_like((rows + 2, ldxn), dt)
    ops.rmsnorm_reduce(xd[:, :dim], gamma.cuda(), 1e-6, xn, rows, slabs=sd if nslab else None, nslab=nslab, slab_stride=(rows + 1) * ld_slab,
                       ld_slab=ld_slab)
    torch.cuda.synchronize()
    xo, xno = xd.cpu(), xn.cpu()
    assert bool(torch.isnan(xo[rows:]).all()) and bool(torch.isnan(xo[:, dim:]).all()), "x guards"
    assert bool(torch.isnan(xno[rows:].float()).all()) and bool(torch.isnan(xno[:, dim:].float()).all()), "xn guards"
    if nslab == 0:
        assert torch.equal(xo[:rows, :dim], x), "nslab = 0: x must be bit-unchanged"
    else:
        ref = x.double() + slabs[:nslab].double().sum(0)
        H.check(f"rmsnorm_reduce slab sum n {nslab}", xo[:rows, :dim], ref,
                H.sum_bound(nslab + 1, x.double().abs() + slabs[:nslab].double().abs().sum(0), ref, torch.float32))
    r, b = H.rmsnorm_ref64(xo[:rows, :dim], gamma, 1e-6, dt)
    H.check(f"rmsnorm_reduce dim {dim} rows {rows} [{dt}]", xno[:rows, :dim], r, b)


# ============================================================================= 5. cv_pack_skinny
def _pack_ref(W, interleave):
    """[N/16][K/32][64 lanes][8]: lane l of k-step ks of tile t holds W[row(t, l & 15)][32 ks + 8 (l >> 4) .. + 7]; rows >= N are zero;
    interleave: tile 2 j = gate rows [16 j, 16 j + 16), tile 2 j + 1 = up rows N / 2 + [16 j, 16 j + 16)."""
    N, K = W.shape
    nt, nks = (N + 15) // 16, K // 32
    t, ks, lane, j = torch.meshgrid(torch.arange(nt), torch.arange(nks), torch.arange(64), torch.arange(8), indexing="ij")
    row = t * 16 + lane % 16
    if interleave:
        row = torch.where(t % 2 == 1, N // 2, 0) + (t // 2) * 16 + lane % 16
    col = ks * 32 + 8 * (lane // 16) + j
    Wz = torch.cat([W, torch.zeros(1, K, dtype=W.dtype)])
    return Wz[torch.where(row < N, row, N), col].reshape(-1)


@gpu
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("N,K,interleave", [(16, 32, False), (100, 64, False), (1, 32, False), (896, 896, False), (64, 128, True), (1792, 896, True),
                                            (1000, 896, False)])
def test_pack_skinny(N, K, interleave, dt):
    from cosyvoice_amd import ops
    g = torch.Generator().manual_seed(N + K)
    W = torch.randn(N, K, generator=g).to(dt)
    Wp = ops.pack_skinny(W.cuda(), interleave=interleave)
    torch.cuda.synchronize()
    assert torch.equal(Wp.cpu().view(torch.int16), _pack_ref(W, interleave).view(torch.int16))


# ============================================================================= 6. cv_skinny_gemm
def _per_wave(K, ksplit):
    return (((K // 32) + ksplit - 1) // ksplit + 3) // 4


# id = the dispatch branch of cv_skinny_gemm (csrc/llm.hip) the case takes: (M, N, K, mode, ksplit, max_wgs)
SKINNY_PLAIN = {
    "exact7-m8": (8, 100, 896, 0, 1, 0), "exact7-m16-ksplit2": (16, 176, 1792, 0, 2, 0), "exact7-m1-mode1": (1, 100, 896, 1, 1, 0),
    "perwave8-m4": (4, 100, 512, 0, 1, 0), "perwave8-m5-k1024": (5, 36, 1024, 0, 1, 0), "perwave8-m9-ksplit4": (9, 100, 4096, 0, 4, 0),
    "perwave8-m1-k32": (1, 17, 32, 0, 1, 0), "perwave8-m16-k96-ksplit4": (16, 50, 96, 0, 4, 0),
    "perwave12-m8": (8, 100, 1536, 0, 1, 0), "perwave12-m16-k1280-mode1": (16, 52, 1280, 1, 1, 0),
    "perwave16-m4": (4, 100, 2048, 0, 1, 0), "perwave16-m9-k1696-mode1": (9, 20, 1696, 1, 1, 0),
    "fallback-gt16-m8-k4864": (8, 100, 4864, 0, 1, 0), "fallback-gt16-m16-k2080-mode1": (16, 40, 2080, 1, 1, 0),
    "perwave8-relu-mode3-m1": (1, 100, 512, 3, 1, 0), "exact7-relu-mode3-m16": (16, 2048, 896, 3, 1, 0),
    "fallback-gt16-relu-mode3-m5": (5, 36, 2112, 3, 1, 0),
    "stream-capped-m8-exact7shape": (8, 1152, 896, 0, 1, 16), "stream-capped-m4-mode1": (4, 1000, 512, 1, 1, 10),
    "stream-capped-m16-ksplit2-perwave12": (16, 600, 3072, 0, 2, 16), "stream-capped-m9-perwave16": (9, 600, 2048, 0, 1, 7),
    "mr2-exact7-m17": (17, 100, 896, 0, 1, 0), "mr2-exact7-m32-mode1": (32, 896, 896, 1, 1, 0),
    "mr2-perwave8-m20": (20, 100, 512, 0, 1, 0), "mr2-perwave8-m32-ksplit2": (32, 36, 2048, 0, 2, 0),
    "mr2-perwave12-m17-oddtiles": (17, 100, 1280, 0, 1, 0), "mr2-perwave12-m32-k1536": (32, 96, 1536, 0, 1, 0),
    "mr2-perwave16-m20": (20, 100, 2048, 0, 1, 0), "mr2-perwave16loop-m32-k4864": (32, 100, 4864, 1, 1, 0),
    "mr2-tpw2-longk-m32-k4864-ksplit4": (32, 896, 4864, 0, 4, 0), "mr2-tpw2-longk-m17-k1280-mode1": (17, 64, 1280, 1, 1, 0),
}


def _skinny_operands(M, N, K, seed, dt):
    g = torch.Generator().manual_seed(seed)
    A = torch.randn(M, K, generator=g).to(dt)
    W = (torch.randn(N, K, generator=g) / K ** 0.5).to(dt)
    bias = torch.randn(N, generator=g)
    res = torch.randn(M, N, generator=g)
    return A, W, bias, res


def _a_dev(A, dt, lda_slack=8):
    """[16 or 32][lda] with the rows >= M zero (the documented precondition) and NaN in the row slack."""
    M, K = A.shape
    buf = H.nan_like((16 if M <= 16 else 32, K + lda_slack), dt)
    buf[:, :K] = 0
    buf[:M, :K] = A.cuda()
    return buf


def _slices(K, ksplit):
    nks = K // 32
    per = (nks + ksplit - 1) // ksplit
    return [(min(nks, s * per) * 32, min(nks, (s + 1) * per) * 32) for s in range(ksplit)]



def _plain_expect(name, dt):
    """Operands and, per output of the case (mode 3: the one 16-bit matrix; modes 0 / 1: every ksplit slab over ITS k range), the float64
    reference and its bound."""
    M, N, K, mode, ksplit, _ = SKINNY_PLAIN[name]
    A, W, bias, res = _skinny_operands(M, N, K, len(name) + K, dt)
    A64, W64 = A.double(), W.double()
    if mode == 3:
        pre = A64 @ W64.t() + bias.double()
        sabs = A64.abs() @ W64.abs().t() + bias.double().abs()
        return A, W, bias, res, [(F.relu(pre), H.sum_bound(K + 1, sabs, F.relu(pre), dt))]
    outs = []
    for s, (k0, k1) in enumerate(_slices(K, ksplit)):
        ref = A64[:, k0:k1] @ W64[:, k0:k1].t()
        sabs = A64[:, k0:k1].abs() @ W64[:, k0:k1].abs().t()
        n = k1 - k0
        if s == 0:
            ref, sabs, n = ref + bias.double(), sabs + bias.double().abs(), n + 1
        if mode == 1:
            ref, sabs, n = ref + res.double(), sabs + res.double().abs(), n + 1
        outs.append((ref, H.sum_bound(n, sabs, ref, torch.float32)))
    return A, W, bias, res, outs


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("name", list(SKINNY_PLAIN))
def test_cpu_skinny_plain_bound_holds_for_torch_fp32(name, dt):
    """torch's fp32 evaluation of what the GPU test asks of the kernel, output by output: each ksplit slab over its k range (+ bias on slab 0,
    + the residual in mode 1), and for mode 3 the ReLU rounded to the 16-bit output type."""
    M, N, K, mode, ksplit, _ = SKINNY_PLAIN[name]
    A, W, bias, res, outs = _plain_expect(name, dt)
    Af, Wf = A.float(), W.float()
    if mode == 3:
        H.check(f"torch fp32 skinny mode 3 {name}", F.relu(Af @ Wf.t() + bias).to(dt), *outs[0])
        return
    for s, (k0, k1) in enumerate(_slices(K, ksplit)):
        t = Af[:, k0:k1] @ Wf[:, k0:k1].t()
        if s == 0:
            t = t + bias
        if mode == 1:
            t = res + t
        H.check(f"torch fp32 skinny mode {mode} {name} slab {s}", t, *outs[s])


def test_cpu_skinny_cases_name_their_branch():
    """The ids state the branch; this recomputes cv_skinny_gemm's dispatch arithmetic for each."""
    for name, (M, N, K, mode, ksplit, max_wgs) in SKINNY_PLAIN.items():
        pw, nt = _per_wave(K, ksplit), (N + 15) // 16
        exact7 = pw == 7 and K // 32 == 28 * ksplit
        if M > 16:
            assert name.startswith("mr2-")
            br = ("tpw2-longk" if 8 < pw <= 10 and nt % 2 == 0 else "exact7" if exact7 else "perwave8" if pw <= 8 else "perwave12" if pw <= 12
                  else "perwave16")
            assert name.startswith("mr2-" + br), (name, br, pw)
        elif pw > 16:
            assert "fallback" in name, (name, pw)
        elif max_wgs and max(1, max_wgs // ksplit) < nt:
            assert name.startswith("stream-capped")
        else:
            assert not name.startswith("stream") and "fallback" not in name
            br = "exact7" if exact7 else "perwave8" if pw <= 8 else "perwave12" if pw <= 12 else "perwave16"
            assert br in name, (name, br, pw)
    assert {c[0] for c in SKINNY_PLAIN.values()} >= {1, 4, 5, 8, 9, 16, 17, 20, 32}


@gpu
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("name", list(SKINNY_PLAIN))
def test_skinny_gemm_plain(name, dt):
    """Modes 0 (every ksplit slab against the float64 product over ITS k range), 1 (in-place residual) and 3 (ReLU, 16-bit) with a bias;
    N is not a multiple of 16 in most cases: the pad columns and the rows >= M of every output stay NaN."""
    from cosyvoice_amd import ops
    M, N, K, mode, ksplit, max_wgs = SKINNY_PLAIN[name]
    A, W, bias, res, outs = _plain_expect(name, dt)
    Wp = ops.pack_skinny(W.cuda())
    Ad = _a_dev(A, dt)
    Mr = 16 if M <= 16 else 32
    ldo = (N + 15) // 16 * 16 + 8
    if mode == 3:
        oa = H.nan_like((Mr + 1, ldo), dt)
        ops.skinny_gemm(Ad, Wp, M, N, K, bias=bias.cuda(), mode=3, out_act=oa, ldoa=ldo, max_wgs=max_wgs)
        torch.cuda.synchronize()
        o = oa.cpu().float()
        H.check(f"skinny mode 3 {name} [{dt}]", o[:M, :N], *outs[0])
        assert bool(torch.isnan(o[M:]).all()) and bool(torch.isnan(o[:, N:]).all()), "mode 3 wrote outside [M][N]"
        return
    of = H.nan_like((ksplit, Mr + 1, ldo), torch.float32)
    if mode == 1:
        of[0, :M, :N] = res.cuda()
    ops.skinny_gemm(Ad, Wp, M, N, K, bias=bias.cuda(), ksplit=ksplit, mode=mode, out_f32=of, ldo=ldo, slab_stride=(Mr + 1) * ldo, max_wgs=max_wgs)
    torch.cuda.synchronize()
    o = of.cpu()
    for s, (ref, bound) in enumerate(outs):
        H.check(f"skinny mode {mode} {name} slab {s} [{dt}]", o[s, :M, :N], ref, bound)
    assert bool(torch.isnan(o[:, M:]).all()) and bool(torch.isnan(o[:, :, N:]).all()), "wrote outside [ksplit][M][N]"


def _swiglu_bound(g, u, bg, bu, dt):
    """h = silu(g) u from pre-activations known to bg, bu: |dh| <= (L_silu bg + rule 3) (|u| + bu) + |silu(g)| bu + one fp32 product rounding +
    half an ulp of the output (test_gemm_modes_gpu.py::test_epilogue_matrix treats SiLU the same way)."""
    s = F.silu(g)
    e32 = (F.silu(g.float()).double() - s).abs().max()
    ds = H.ACT_LIPSCHITZ["SILU"] * bg + 4.0 * torch.maximum(e32, H.EPS32 * s.abs())
    h = s * u
    return h, ds * (u.abs() + bu) + s.abs() * bu + H.EPS32 * h.abs() + 0.5 * H.ulp(h, dt)


def _swiglu32(pre, h2, dt):
    """torch fp32: silu(gate) * up of an fp32 pre-activation [gate | up], rounded to the output type."""
    return (F.silu(pre[:, :h2]) * pre[:, h2:]).to(dt)


SWIGLU = {
    "exact7-m8": (8, 128, 896, 0), "perwave8-m1-k512": (1, 64, 512, 0), "perwave8-m16-k1024": (16, 96, 1024, 0),
    "fallback-tpw2-perwave12-m5-k1536": (5, 64, 1536, 0), "fallback-tpw2-m9-k4864": (9, 64, 4864, 0),
    "stream-capped-m4": (4, 1024, 896, 6), "stream-capped-m16-k512": (16, 640, 512, 4),
}


def _swiglu_expect(name, dt):
    M, N, K, _ = SWIGLU[name]                             # N = gate rows + up rows
    A, W, bias, _ = _skinny_operands(M, N, K, len(name) + K, dt)
    A64, W64, b64 = A.double(), W.double(), bias.double()
    pre = A64 @ W64.t() + b64
    pb = H.sum_bound(K + 1, A64.abs() @ W64.abs().t() + b64.abs(), pre, torch.float32)
    h2 = N // 2
    ref, bound = _swiglu_bound(pre[:, :h2], pre[:, h2:], pb[:, :h2], pb[:, h2:], dt)
    return A, W, bias, ref, bound


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("name", list(SWIGLU))
def test_cpu_skinny_swiglu_bound_holds_for_torch_fp32(name, dt):
    A, W, bias, ref, bound = _swiglu_expect(name, dt)
    H.check(f"torch fp32 skinny mode 2 {name}", _swiglu32(A.float() @ W.float().t() + bias, W.shape[0] // 2, dt), ref, bound)


@gpu
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("name", list(SWIGLU))
def test_skinny_gemm_swiglu(name, dt):
    """Mode 2: interleaved [gate16 | up16] tiles, out_act[m][16 pair + i] = silu(g) u, with a bias in packed column order."""
    from cosyvoice_amd import ops
    M, N, K, max_wgs = SWIGLU[name]
    A, W, bias, ref, bound = _swiglu_expect(name, dt)
    Wp = ops.pack_skinny(W.cuda(), interleave=True)
    Ad = _a_dev(A, dt)
    h2 = N // 2
    ldoa = h2 + 8
    oa = H.nan_like((17, ldoa), dt)
    # the bias is indexed by PACKED column: tile 2 j = gate rows 16 j .., tile 2 j + 1 = up rows
    t = torch.arange(N) // 16
    src = torch.where(t % 2 == 1, h2, 0) + (t // 2) * 16 + torch.arange(N) % 16
    ops.skinny_gemm(Ad, Wp, M, N, K, bias=bias[src].cuda(), mode=2, out_act=oa, ldoa=ldoa, max_wgs=max_wgs)
    torch.cuda.synchronize()
    o = oa.cpu().float()
    H.check(f"skinny mode 2 {name} [{dt}]", o[:M, :h2], ref, bound)
    assert bool(torch.isnan(o[M:]).all()) and bool(torch.isnan(o[:, h2:]).all()), "mode 2 wrote outside [M][N / 2]"


NORM_CASES = {   # (M, N, K, nslab, mode, max_wgs, with nx_out): tpr 64 / 32 / 16 by M, exact7 at K = 896 for M > 4
    "tpr64-m1-k896-nslab0": (1, 100, 896, 0, 0, 0, False), "tpr64-m4-k1024-nslab4": (4, 100, 1024, 4, 0, 0, True),
    "tpr32-m5-k896-exact7-nslab1": (5, 100, 896, 1, 0, 0, True), "tpr32-m8-k512-nslab2": (8, 36, 512, 2, 0, 0, True),
    "tpr16-m9-k896-exact7-nslab4": (9, 1152, 896, 4, 0, 0, True), "tpr16-m16-k64-nslab0": (16, 100, 64, 0, 0, 0, True),
    "tpr16-m16-k1024-nslab2-ksplit": (16, 100, 1024, 2, 0, 0, True),
    "swiglu-m8-k896-nslab4": (8, 128, 896, 4, 2, 0, True), "swiglu-m3-k512-nslab1": (3, 64, 512, 1, 2, 0, False),
    "stream-capped-m8-k896-nslab4": (8, 1152, 896, 4, 0, 16, True), "stream-capped-swiglu-m16-k896-nslab2": (16, 1024, 896, 2, 2, 6, True),
}


def _norm_inputs(M, K, nslab, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g)
    x[0] *= 30.0
    slabs = torch.randn(max(nslab, 1), M, K, generator=g)
    gamma = 1.0 + 0.3 * torch.randn(K, generator=g)
    return x, slabs, gamma


def _norm_expect(name, dt):
    """Inputs of a prologue case and what is asked of its outputs: v64 / vb for nx_out (rule 2, n = nslab + 1) and, per output (mode 0: every
    ksplit slab; mode 2: the one SwiGLU matrix), the float64 reference from the UNROUNDED float64 operand and its bound."""
    M, N, K, nslab, mode, _, _ = NORM_CASES[name]
    ksplit = 2 if "ksplit" in name else 1
    _, W, bias, _ = _skinny_operands(M, N, K, len(name) + K, dt)
    x, slabs, gamma = _norm_inputs(M, K, nslab, len(name))
    v64 = x.double() + slabs[:nslab].double().sum(0)
    dv = H.sum_bound(nslab + 1, x.double().abs() + slabs[:nslab].double().abs().sum(0), v64, torch.float32)
    # the operand.  a_ref = rmsnorm64(v64) gamma.  The kernel normalises ITS fp32 row sums v' (|v' - v64| <= dv, the slab-sum bound) within the
    # RMSNorm bound; f(v) = v r(v), r = (mean(v^2) + eps)^-1/2 moves by |df_i| <= r |dv_i| + |f_i| ||dv|| / ||v|| to first order (dr = -r^3
    # <v, dv> / dim and r^2 <= dim / ||v||^2); twice that covers the higher orders
    a_ref, bA = H.rmsnorm_ref64(v64, gamma, 1e-6, dt)
    rstd = torch.rsqrt((v64 * v64).mean(-1, keepdim=True) + 1e-6)
    bA = bA + 2.0 * (dv * rstd * gamma.double().abs() + a_ref.abs() * (dv.norm(dim=-1, keepdim=True) / v64.norm(dim=-1, keepdim=True).clamp_min(1e-30)))
    W64 = W.double()
    if mode == 2:
        pre = a_ref @ W64.t()
        pb = bA @ W64.abs().t() + H.sum_bound(K, (a_ref.abs() + bA) @ W64.abs().t(), pre, torch.float32)
        h2 = N // 2
        outs = [_swiglu_bound(pre[:, :h2], pre[:, h2:], pb[:, :h2], pb[:, h2:], dt)]
    else:
        outs = []
        for s, (k0, k1) in enumerate(_slices(K, ksplit)):
            ref = a_ref[:, k0:k1] @ W64[:, k0:k1].t() + (bias.double() if s == 0 else 0)
            sa = (a_ref[:, k0:k1].abs() + bA[:, k0:k1]) @ W64[:, k0:k1].abs().t() + (bias.double().abs() if s == 0 else 0)
            outs.append((ref, bA[:, k0:k1] @ W64[:, k0:k1].abs().t() + H.sum_bound(k1 - k0 + 1, sa, ref, torch.float32)))
    return W, bias, x, slabs, gamma, v64, dv, outs, ksplit


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("name", list(NORM_CASES))
def test_cpu_skinny_norm_prologue_bound_holds_for_torch_fp32(name, dt):
    """torch fp32: the slab sum term by term, RMSNorm in fp32, the operand ROUNDED to the 16-bit type, then the fp32 product (per ksplit slab,
    + bias) or SwiGLU: the composed bound, with its factor 2 on the first-order term, holds for plain fp32 arithmetic."""
    M, N, K, nslab, mode, _, _ = NORM_CASES[name]
    W, bias, x, slabs, gamma, v64, dv, outs, ksplit = _norm_expect(name, dt)
    v = x.clone()
    for s in range(nslab):
        v = v + slabs[s]
    H.check(f"torch fp32 prologue row sum {name}", v, v64, dv)
    a = (v * torch.rsqrt((v * v).mean(-1, keepdim=True) + 1e-6) * gamma).to(dt).float()
    Wf = W.float()
    if mode == 2:
        H.check(f"torch fp32 prologue + mode 2 {name}", _swiglu32(a @ Wf.t(), N // 2, dt), *outs[0])
        return
    for s, (k0, k1) in enumerate(_slices(K, ksplit)):
        t = a[:, k0:k1] @ Wf[:, k0:k1].t()
        H.check(f"torch fp32 prologue + mode 0 {name} slab {s}", t + bias if s == 0 else t, *outs[s])


@gpu
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("name", list(NORM_CASES))
def test_skinny_gemm_norm_prologue(name, dt):
    """Fused prologue: v = nx + sum of slabs (stored to nx_out: rule 2, n = nslab + 1), A = T(rmsnorm(v) gamma) known to the RMSNorm bound b_A,
    out = A W^T: |d out| <= b_A |W|^T + rule 2 with n = K."""
    from cosyvoice_amd import ops
    M, N, K, nslab, mode, max_wgs, with_out = NORM_CASES[name]
    W, bias, x, slabs, gamma, v64, dv, outs, ksplit = _norm_expect(name, dt)
    ldnx, ld_slab = K + 4, K + 8
    xd = H.nan_like((17, ldnx), torch.float32)
    xd[:M, :K] = x.cuda()
    sd = H.nan_like((max(nslab, 1), 17, ld_slab), torch.float32)
    sd[:, :M, :K] = slabs.cuda()
    xo = H.nan_like((17, ldnx), torch.float32) if with_out else None
    norm = dict(x=xd, gamma=gamma.cuda(), eps=1e-6, x_out=xo, slabs=sd if nslab else None, nslab=nslab, slab_stride=17 * ld_slab, ld_slab=ld_slab)
    Wp = ops.pack_skinny(W.cuda(), interleave=(mode == 2))
    dummy = torch.zeros(16, 8, dtype=dt, device="cuda")
    if mode == 2:
        h2 = N // 2
        oa = H.nan_like((17, h2 + 8), dt)
        ops.skinny_gemm(dummy, Wp, M, N, K, mode=2, out_act=oa, ldoa=h2 + 8, norm=norm, max_wgs=max_wgs)
    else:
        ldo = (N + 15) // 16 * 16 + 8
        of = H.nan_like((ksplit, 17, ldo), torch.float32)
        ops.skinny_gemm(dummy, Wp, M, N, K, bias=bias.cuda(), ksplit=ksplit, out_f32=of, ldo=ldo, slab_stride=17 * ldo, norm=norm, max_wgs=max_wgs)
    torch.cuda.synchronize()
    if with_out:
        xoc = xo.cpu()
        assert bool(torch.isnan(xoc[M:]).all()) and bool(torch.isnan(xoc[:, K:]).all()), "nx_out guards"
        H.check(f"prologue nx_out {name}", xoc[:M, :K], v64, dv)
    assert torch.equal(xd.cpu()[:M, :K], x), "nx is read-only"
    if mode == 2:
        o = oa.cpu().float()
        H.check(f"prologue + mode 2 {name} [{dt}]", o[:M, :h2], *outs[0])
        assert bool(torch.isnan(o[M:]).all()) and bool(torch.isnan(o[:, h2:]).all())
        return
    o = of.cpu()
    for s, (ref, bound) in enumerate(outs):
        H.check(f"prologue + mode 0 {name} slab {s} [{dt}]", o[s, :M, :N], ref, bound)
    assert bool(torch.isnan(o[:, M:]).all()) and bool(torch.isnan(o[:, :, N:]).all())


SPLIT_CASES = {"m3": (3, 896), "m8": (8, 896), "m16": (16, 896), "m16-k512": (16, 512), "mr2-m17": (17, 896), "mr2-m32": (32, 896),
               "mr2-m20-k1024-perwave8": (20, 1024)}
SPLIT_KP, SPLIT_N2 = 512, 256          # the producer's K; the consumer's 128 gate + 128 up rows


def _split_operands(name, dt):
    M, K = SPLIT_CASES[name]
    A, Wo, _, res = _skinny_operands(M, K, SPLIT_KP, len(name), dt)
    res[0] *= 20.0
    g = torch.Generator().manual_seed(M)
    Wgu = (torch.randn(SPLIT_N2, K, generator=g) / K ** 0.5).to(dt)
    return A, Wo, res, Wgu


def _split_checks(name, dt, who, A, Wo, res, Wgu, o, xb, ss, o2):
    """What is asked of the four outputs (CPU tensors: o (M, K) fp32, xb (M, K) 16-bit, ss (K / 16, M) fp32, o2 (M, 128)), whoever made them.
    Each stage is held to the float64 evaluation of ITS OWN inputs as they were stored by the stage before."""
    M, K = SPLIT_CASES[name]
    nparts, h2 = K // 16, SPLIT_N2 // 2
    ref = res.double() + A.double() @ Wo.double().t()
    sabs = res.double().abs() + A.double().abs() @ Wo.double().abs().t()
    H.check(f"{who} split producer out {name} [{dt}]", o, ref, H.sum_bound(SPLIT_KP + 1, sabs, ref, torch.float32))
    assert torch.equal(xb, o.double().to(dt)), "xb_out = T(out), bit-exact"
    sq = (o.double() ** 2).view(M, nparts, 16).sum(-1).t()                               # (parts, M)
    H.check(f"{who} split producer ss_part {name}", ss, sq, H.sum_bound(16, sq, sq, torch.float32))
    X = xb.double()
    rstd = torch.rsqrt(ss.double().sum(0) / K + torch.tensor(1e-6, dtype=torch.float32).double())[:, None]
    raw = X @ Wgu.double().t()
    pre = raw * rstd
    rb = H.sum_bound(K, X.abs() @ Wgu.double().abs().t(), raw, torch.float32) * rstd + (nparts / 2 + 5) * H.EPS32 * pre.abs()
    ref2, bound2 = _swiglu_bound(pre[:, :h2], pre[:, h2:], rb[:, :h2], rb[:, h2:], dt)
    H.check(f"{who} split consumer {name} [{dt}]", o2, ref2, bound2)


@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("name", list(SPLIT_CASES))
def test_cpu_skinny_split_norm_bounds_hold_for_torch_fp32(name, dt):
    """torch fp32 through both halves: out = res + A W^T, xb = T(out), the 16-column partial sums of squares, then rsqrt(sum / K + eps) applied
    to the fp32 product of xb with the gate / up weights and SwiGLU: every bound of the GPU test, its (n_rs / 2 + 5) 2^-23 included."""
    M, K = SPLIT_CASES[name]
    A, Wo, res, Wgu = _split_operands(name, dt)
    o = res + A.float() @ Wo.float().t()
    xb = o.to(dt)
    ss = (o * o).view(M, K // 16, 16).sum(-1).t().contiguous()
    rstd = torch.rsqrt(ss.sum(0) / K + 1e-6)[:, None]
    o2 = _swiglu32((xb.float() @ Wgu.float().t()) * rstd, SPLIT_N2 // 2, dt)
    _split_checks(name, dt, "torch fp32", A, Wo, res, Wgu, o, xb, ss, o2)


@gpu
@pytest.mark.parametrize("dt", DTS, ids=DT_IDS)
@pytest.mark.parametrize("name", list(SPLIT_CASES))
def test_skinny_split_norm_producer_consumer(name, dt):
    """Producer (mode 1 + xb_out + ss_part): out = res + A W^T (rule 2), xb = T(out) bit-exact from the fp32 the op stored, ss_part[tile][m] =
    the sum of that tile's 16 squares (rule 2, n = 16).  Consumer (mode 2 + rs_part, M <= 16 and the two-row-group MR = 2 kernels):
    gate / up scaled by rsqrt(sum of partials / K + eps) — the sum of n_rs partials and / K + eps err by (n_rs + 4) 2^-23 relative, half
    of it through rsqrt, + 2 ulp of rsqrtf + the product: r = (n_rs / 2 + 5) 2^-23 relative on top of rule 2."""
    from cosyvoice_amd import ops
    M, K = SPLIT_CASES[name]
    Hd, N2 = K, SPLIT_N2
    Mr = 16 if M <= 16 else 32
    A, Wo, res, Wgu = _split_operands(name, dt)
    of = H.nan_like((Mr + 1, Hd + 8), torch.float32)
    of[:M, :Hd] = res.cuda()
    xb = H.nan_like((Mr + 1, Hd + 8), dt)
    xb[M:Mr, :Hd] = 0                                       # the consumer's A rows >= M must be finite (documented precondition)
    nparts = Hd // 16
    ss = H.nan_like((nparts + 1, Mr), torch.float32)
    ops.skinny_gemm(_a_dev(A, dt), ops.pack_skinny(Wo.cuda()), M, Hd, SPLIT_KP, mode=1, out_f32=of, ldo=Hd + 8, split_out=dict(xb=xb, ss=ss))
    h2 = N2 // 2
    oa = H.nan_like((Mr + 1, h2 + 8), dt)
    ops.skinny_gemm(xb, ops.pack_skinny(Wgu.cuda(), interleave=True), M, N2, K, mode=2, out_act=oa, ldoa=h2 + 8,
                    split_in=dict(rs=ss, n=nparts, eps=1e-6))        # the NaN guards of ss stay: not read
    torch.cuda.synchronize()
    o, xbc, ssc, o2 = of.cpu(), xb.cpu(), ss.cpu(), oa.cpu().float()
    assert bool(torch.isnan(o[M:]).all()) and bool(torch.isnan(o[:, Hd:]).all()) and bool(torch.isnan(xbc[Mr:].float()).all())
    assert bool(torch.isnan(xbc[:, Hd:].float()).all()) and bool((xbc[M:Mr, :Hd] == 0).all()), "xb_out guards"
    assert bool(torch.isnan(ssc[nparts:]).all()) and bool(torch.isnan(ssc[:, M:]).all()), "ss_part guards"
    assert bool(torch.isnan(o2[M:]).all()) and bool(torch.isnan(o2[:, h2:]).all()), "consumer wrote outside [M][N / 2]"
    _split_checks(name, dt, "device", A, Wo, res, Wgu, o[:M, :Hd], xbc[:M, :Hd], ssc[:nparts, :M], o2[:M, :h2])
