"""No GPU needed: the ragged-vocoder additions to the ABI (struct handshake, argument validation before any launch) and the RULE the
kernels implement, pinned on the CPU oracle: in a padded batch it is enough that every convolution reads zeros past the row's own length
at that stage and that the STFT / iSTFT run on the row's own extent — whatever else lies past the length never reaches the valid part."""
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F

from cosyvoice_amd.config import HiftConfig
from cosyvoice_amd.weights import fold_weight_norm, hift_downsample_plan, hift_state_dict

HERE = os.path.dirname(os.path.abspath(__file__))


# ----------------------------------------------------------------------------- ABI
def test_struct_handshake_with_the_length_fields():
    from cosyvoice_amd import _lib as L
    lib = L.lib()   # raises on a size mismatch between the header's structs and the ctypes mirrors
    assert lib.cv_sizeof_gemm_params() == ctypes.sizeof(L.GemmParams)
    assert lib.cv_sizeof_hift_decode_desc() == ctypes.sizeof(L.HiftDecodeDesc)
    gp = [n for n, _ in L.GemmParams._fields_]
    assert gp[-5:] == ["len_base", "a_len_mul", "a_len_add", "m_len_mul", "m_len_add"]       # trailing: every older field keeps its offset
    assert [n for n, _ in L.HiftDecodeDesc._fields_][-1] == "lens"
    p, d = L.GemmParams(), L.HiftDecodeDesc()
    assert not p.len_base and (p.a_len_mul, p.a_len_add, p.m_len_mul, p.m_len_add) == (0, 0, 0, 0) and not d.lens   # zero-initialised = off
    hdr = open(os.path.join(HERE, "..", "include", "cosyvoice_amd.h")).read()
    assert re.search(r"const int32_t\* len_base; int32_t a_len_mul, a_len_add, m_len_mul, m_len_add;\s*} cv_gemm_params;", hdr)
    assert re.search(r"const int32_t\* lens;[^}]*} cv_hift_decode_desc;", hdr)


def test_no_new_export_for_the_ragged_path():
    from cosyvoice_amd import _lib as L
    hdr = open(os.path.join(HERE, "..", "include", "cosyvoice_amd.h")).read()
    assert set(re.findall(r"\b(cv_[a-z0-9_]+)\s*\(", hdr)) == set(L.EXPORTS)
    assert not [n for n in L.EXPORTS if "ragged" in n or "lens" in n]


def _gemm_ok_but_for_lengths(L):
    p = L.GemmParams()
    p.M, p.N, p.K, p.batch, p.dtype = 64, 8, 32, 2, L.CV_BF16
    p.A, p.W, p.out_f32, p.lda, p.ldw, p.ldo32 = 16, 16, 16, 32, 32, 8
    return p


def test_cv_gemm_rejects_inconsistent_length_arguments_before_launching():
    from cosyvoice_amd import _lib as L
    lib = L.lib()
    null = ctypes.c_void_p(None)
    p = _gemm_ok_but_for_lengths(L)
    p.a_len_mul = 1                                    # multipliers without the length array
    assert lib.cv_gemm(ctypes.byref(p), null) == -1
    p = _gemm_ok_but_for_lengths(L)
    p.m_len_add = 3
    assert lib.cv_gemm(ctypes.byref(p), null) == -1
    p = _gemm_ok_but_for_lengths(L)
    p.len_base = 16                                    # a length array that bounds nothing
    assert lib.cv_gemm(ctypes.byref(p), null) == -1
    p.a_len_mul = -1                                   # negative multiplier
    assert lib.cv_gemm(ctypes.byref(p), null) == -1
    p.a_len_mul, p.len_base = 1, 18                    # int32 array not 4-byte aligned
    assert lib.cv_gemm(ctypes.byref(p), null) == -1
    p.len_base, p.batch, p.batch_inner = 16, 4, 2      # two-level batch: which index the length belongs to is not defined
    assert lib.cv_gemm(ctypes.byref(p), null) == -3
    p.batch, p.batch_inner, p.out_mode = 2, 0, L.OUT_QKV
    assert lib.cv_gemm(ctypes.byref(p), null) < 0


def _desc(L, T=4, us=(4, 3), hop=4):
    """A descriptor that passes check_hift_desc (dummy non-null pointers, never dereferenced on the rejected paths)."""
    keep = []
    d = L.HiftDecodeDesc()
    d.dtype, d.gemm_dtype, d.B, d.T, d.n_stages, d.n_kernels, d.stft_ld, d.hop = L.CV_F32, L.CV_F32, 2, T, len(us), 1, 20, hop
    rows = T
    stages = (L.HiftStage * len(us))()
    for i, u in enumerate(us):
        rows *= u
        g = stages[i]
        ph = (L.HiftPhase * u)()
        un = (L.HiftResunit * 1)()
        rb = (L.HiftResblock * 1)()
        rb[0].units, rb[0].n_units = un, 1
        xa = (ctypes.c_void_p * 1)(16)
        keep += [ph, un, rb, xa]
        g.phases, g.u, g.rbs, g.xa = ph, u, rb, xa
        g.source_rb.units, g.source_rb.n_units = un, 1
        g.t_out, g.c = rows + (1 if i == len(us) - 1 else 0), 8
        for f in ("x32", "r0", "r1", "ta", "ra", "acc0", "acc1", "si0", "si1", "out"):
            setattr(g, f, 16)
    d.S = rows * hop
    d.stages = stages
    d.conv_pre.w = d.conv_post.w = 16
    d.mel_cl = d.s = d.stft = d.a_pre = d.post = d.wav = 16
    keep.append(stages)
    return d, keep


def test_cv_hift_decode_rejects_inconsistent_ragged_descriptors_before_launching():
    from cosyvoice_amd import _lib as L
    lib = L.lib()
    null = ctypes.c_void_p(None)
    for fn in (lib.cv_hift_decode_enqueue, lib.cv_hift_decode):
        d, keep = _desc(L)
        d.lens = 18                                    # misaligned int32 array
        assert fn(ctypes.byref(d), null) == -1
        d, keep = _desc(L)
        d.lens, d.S = 16, d.S + 4                      # S is not T * prod(u) * hop: the per-row sample counts could not be derived
        assert fn(ctypes.byref(d), null) == -1
        d, keep = _desc(L)
        d.lens = 16
        d.stages[0].t_out += 1                         # a stage that is not T * prod(u) rows long
        assert fn(ctypes.byref(d), null) == -1
        d, keep = _desc(L)
        d.lens = 16
        d.stages[1].t_out -= 1                         # last stage without the reflect-pad row
        assert fn(ctypes.byref(d), null) == -1
    d, keep = _desc(L)
    d.lens, d.S = 16, d.S + 4
    out = ctypes.c_void_p()
    assert lib.cv_hift_decode_graph_create(ctypes.byref(d), ctypes.c_void_p(16), ctypes.byref(out)) == -1 and not out.value


def test_python_composed_decode_has_no_ragged_form():
    from cosyvoice_amd.hift import HiFTGenerator
    m = HiFTGenerator.__new__(HiFTGenerator)
    m.use_stage_abi = False
    with pytest.raises(RuntimeError, match="no ragged form"):
        m._decode_cl({}, 2, 8, None, ragged=True)


# ----------------------------------------------------------------------------- the rule, on the CPU oracle
def _masked_decode(sd, cfg, x, s, lens, junk):
    """oracle.hift.decode over a PADDED batch (x (B,80,T), s (B,1,T*up), frame counts ``lens``) with exactly the six per-utterance rules
    of the ragged kernels and nothing else: every conv1d / conv_transpose1d input is zeroed past the row's own length at that stage, the
    STFT / iSTFT run on the row's own extent — and after EVERY op everything past the row's length is overwritten with ``junk``."""
    from oracle import hift as oh
    B, _, T = x.shape
    up = cfg.total_upsample

    def past(t, L, v):
        t = t.clone()
        for b, n in enumerate(L):
            t[b, :, n:] = v
        return t

    conv = lambda t, L, w, b, **kw: F.conv1d(past(t, L, 0.0), w, b, **kw)

    def resblock(name, t, k, dils, L):
        for j, dl in enumerate(dils):
            xt = past(oh.snake(t, sd[f"{name}.activations1.{j}.alpha"]), L, junk)
            xt = past(conv(xt, L, fold_weight_norm(sd, f"{name}.convs1.{j}"), sd[f"{name}.convs1.{j}.bias"], dilation=dl, padding=oh.get_padding(k, dl)), L, junk)
            xt = past(oh.snake(xt, sd[f"{name}.activations2.{j}.alpha"]), L, junk)
            xt = conv(xt, L, fold_weight_norm(sd, f"{name}.convs2.{j}"), sd[f"{name}.convs2.{j}.bias"], dilation=1, padding=oh.get_padding(k, 1))
            t = past(xt + t, L, junk)
        return t

    Fp = T * up // cfg.hop_len + 1
    Fl = [n * up // cfg.hop_len + 1 for n in lens]
    s_stft = torch.full((B, cfg.n_fft + 2, Fp), junk)
    for b, n in enumerate(lens):
        re, im = oh.stft(cfg, s[b, :, :n * up])
        s_stft[b, :, :Fl[b]] = torch.cat([re, im], dim=1)[0]
    L = list(lens)
    x = past(conv(past(x, L, junk), L, fold_weight_norm(sd, "conv_pre"), sd["conv_pre.bias"], padding=3), L, junk)
    nk, nu = len(cfg.resblock_kernel_sizes), len(cfg.upsample_rates)
    plan = hift_downsample_plan(cfg)
    for i in range(nu):
        x = past(F.leaky_relu(x, cfg.lrelu_slope), L, junk)
        u, k = cfg.upsample_rates[i], cfg.upsample_kernel_sizes[i]
        x = F.conv_transpose1d(past(x, L, 0.0), fold_weight_norm(sd, f"ups.{i}"), sd[f"ups.{i}.bias"], stride=u, padding=(k - u) // 2)
        L = [n * u for n in L]
        if i == nu - 1:
            x = F.pad(x, (1, 0), mode="reflect")
            L = [n + 1 for n in L]
        x = past(x, L, junk)
        stride, ks, pad = plan[i]
        si = conv(s_stft, Fl, sd[f"source_downs.{i}.weight"], sd[f"source_downs.{i}.bias"], stride=stride, padding=pad)
        assert si.shape[2] == x.shape[2]
        si = resblock(f"source_resblocks.{i}", past(si, L, junk), cfg.source_resblock_kernel_sizes[i], cfg.source_resblock_dilation_sizes[i], L)
        x = past(x + si, L, junk)
        xs = None
        for j in range(nk):
            r = resblock(f"resblocks.{i * nk + j}", x, cfg.resblock_kernel_sizes[j], cfg.resblock_dilation_sizes[j], L)
            xs = r if xs is None else xs + r
        x = past(xs / nk, L, junk)
    x = past(F.leaky_relu(x), L, junk)
    x = past(conv(x, L, fold_weight_norm(sd, "conv_post"), sd["conv_post.bias"], padding=3), L, junk)
    nb = cfg.n_fft // 2 + 1
    outs = []
    for b, n in enumerate(L):
        y = oh.istft(cfg, torch.exp(x[b:b + 1, :nb, :n]), torch.sin(x[b:b + 1, nb:, :n]))
        outs.append(torch.clamp(y, -cfg.audio_limit, cfg.audio_limit)[0])
    return outs


@pytest.mark.parametrize("tag,cfg", [("tiny", HiftConfig.tiny()), ("v1", HiftConfig.v1())])
def test_read_masking_at_the_six_places_reproduces_batch1_decode(tag, cfg):
    """17- and 5-frame utterances inside a 29-frame padded batch.  Against the oracle's batch-1 decode of each utterance alone the masked
    batch differs by fp32 rounding of the CPU convolution only (torch picks its algorithm by shape: 1e-6, the project's "batch row == single
    run" tolerance), and it does not depend on what the padding holds: bit-equal between junk 0 and junk 37.5."""
    from oracle import hift as oh
    sd = hift_state_dict(cfg)
    up = cfg.total_upsample
    T, lens = 29, [17, 29, 5]
    g = torch.Generator().manual_seed(4)
    x = torch.clamp(torch.randn(len(lens), 80, T, generator=g) * 2 - 6, -11.5, 2.0)
    s = torch.randn(len(lens), 1, T * up, generator=g) * 0.05
    with torch.no_grad():
        a = _masked_decode(sd, cfg, x, s, lens, 0.0)
        b = _masked_decode(sd, cfg, x, s, lens, 37.5)
        for i, n in enumerate(lens):
            ref = oh.decode(sd, cfg, x[i:i + 1, :, :n], s[i:i + 1, :, :n * up])[0]
            assert a[i].shape == ref.shape == (n * up,)
            err = (a[i] - ref).abs().max().item()
            print(f"masked padded batch, {tag}, row {i} ({n} of {T} frames): vs batch-1 oracle {err:.2e}")
            assert err < 1e-6
            assert torch.equal(a[i], b[i])


# ----------------------------------------------------------------------------- the built GEMM kernels: no scratch, occupancy kept
def _gfx950_code_objects(blob):
    """the gfx950 ELF images inside the clang offload bundles of a linked library"""
    import struct
    magic, pos = b"__CLANG_OFFLOAD_BUNDLE__", 0
    while True:
        i = blob.find(magic, pos)
        if i < 0:
            return
        n, = struct.unpack_from("<Q", blob, i + 24)
        p = i + 32
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", blob, p)
            triple = blob[p + 24:p + 24 + tl].decode()
            p += 24 + tl
            if "gfx950" in triple and size:
                yield blob[i + off:i + off + size]
        pos = i + 24


def _kernel_descriptors(elf):
    """kernel name -> (scratch bytes per lane, registers per lane) from the 64-byte amdhsa kernel descriptors (<name>.kd symbols):
    private_segment_fixed_size at byte 4; compute_pgm_rsrc1[5:0] = granulated VGPR count (unified VGPR + AGPR file, granule 8)."""
    import struct
    assert elf[:4] == b"\x7fELF"
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum, _ = struct.unpack_from("<HHH", elf, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", elf, shoff + k * shentsize) for k in range(shnum)]
    out = {}
    for s in secs:
        if s[1] not in (2, 11):   # SHT_SYMTAB / SHT_DYNSYM
            continue
        strs = secs[s[6]]
        for k in range(s[5] // 24):
            name_off, _, _, shndx, value, _ = struct.unpack_from("<IBBHQQ", elf, s[4] + k * 24)
            name = elf[strs[4] + name_off:elf.index(b"\0", strs[4] + name_off)].decode()
            if name.endswith(".kd") and 0 < shndx < shnum:
                o = secs[shndx][4] + value - secs[shndx][3]
                scratch, = struct.unpack_from("<I", elf, o + 4)
                rsrc1, = struct.unpack_from("<I", elf, o + 48)
                out[name[:-3]] = (scratch, ((rsrc1 & 63) + 1) * 8)
    return out


def test_gemm_kernels_have_no_scratch_and_the_presplit_kernels_keep_four_waves():
    """The per-batch length is a scalar load per workgroup, not registers per lane: in the library as built, no cv_gemm kernel uses scratch
    memory, and the pre-split bf16x3 kernels — the decoder's convs, which hide their staging latency by occupancy — still
    fit 4 waves per SIMD (512 registers per SIMD lane / 4 = 128, VGPRs + AGPRs)."""
    from cosyvoice_amd import _lib as L
    L.lib()
    ks = {}
    for co in _gfx950_code_objects(open(L.LIB_PATH, "rb").read()):
        ks.update({k: v for k, v in _kernel_descriptors(co).items() if re.search(r"gemm_kernel|conv_win_kernel", k)})
    assert len(ks) >= 18, sorted(ks)   # 3 tiles x 3 dtypes + 2 tiles x (plain, pre-split) bf16x3 + 5 window-kernel shapes
    assert all(scratch == 0 for scratch, _ in ks.values()), {k: v for k, v in ks.items() if v[0]}
    presplit = {k: v for k, v in ks.items() if re.search(r"gemm_kernelILi0E.*Lb1ELb1EEE", k)}     # <CV_F32, ..., X3 = true, PS = true>
    assert len(presplit) == 2 and all(regs <= 128 for _, regs in presplit.values()), presplit
