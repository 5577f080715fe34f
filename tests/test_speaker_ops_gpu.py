"""Op-level parity of the speaker encoder's kernels (csrc/speaker.hip: cv_spk_power, cv_spk_log_cmn, cv_spk_conv, cv_spk_cam_gate,
cv_spk_stats_pool) through the C ABI against float64 references computed on the CPU from the fp32 operands, element-wise (H.check: no element,
row or case is left out), by the rules stated at the top of tests/test_helper_kernels_gpu.py.

Buffers.  Every buffer has NaN slack: input rows at and past a sequence's length hold NaN, so do the columns [cin, ldx) of every input row, GUARD
rows follow every sequence (the batch strides are larger than T rows), guard columns surround an output window, and outputs are NaN before the
launch.  After it the rows [len, T) of the op's window are exactly 0, everything outside rows x columns still holds what it held (NaN, or the
data of a wide block buffer, bit for bit), and read-only inputs are compared bit for bit.

Bounds (H.spk_*_ref64; nothing is fitted to the kernels).
  conv      rule 2 with n = kf kt cin, plus one term each for the prologue fma, the bias, the residual and the gate product, on sum|A w| + |bias|
            + |res|, times |gate|.  ReLU is 1-Lipschitz.  Padded taps contribute 0, never relu(shift): the reference zero-pads AFTER the prologue.
  psum      each 4-row group sum against the float64 sum of the rows that launch stored: rule 2 with n = 4.
  gate      rule 2 on the two group sums (n = the number of groups each spans), half an ulp for each division and the sum of the context; pushed
            through |w1| with rule 2, n = 128 + 1; through |w2|, n = 64 + 1; the sigmoid is 1/4-Lipschitz and pays rule 3 (expf, reciprocal).
  pooling   a_t = relu(x_t scale + shift) (da_t = 2^-24 |a_t|, the fma's rounding; 0 without the prologue), n = len rows:
                dmu  = ((n + 2) 2^-23 sum|a| + sum da) / n + 2^-24 |mu|          rule 2 on the sum, the division
                dd_t = dmu + da_t + half an ulp of d_t                           d_t = a_t - mu
                dq   = (n + 2) 2^-23 q + 2 sum |d_t| dd_t                        q = sum d^2: rule 2 on the squares + d(d^2) = 2 |d| dd
                dvar = dq / (n - 1) + 2^-24 var
                dstd = min(dvar / (2 std), sqrt(dvar)) + rule 3 for sqrtf        |sqrt(v + e) - sqrt(v)| <= e / (2 sqrt v) and <= sqrt e
            to first order; the bound is 2 dmu for the mean and the same with 2 dvar for the std.  It is NOT shift-invariant (dmu carries sum|a|):
            the kernel holds the mean in one fp32 and the +30 case (every row offset by 30) is held to what that allows.  n >= 2 is a
            precondition (include/cosyvoice_amd.h): the unbiased std of one frame is 0 / 0 in the reference as well.
  power     rule 2 with n = 2.
  log + CMN rule 3 for logf (e32: torch's fp32 log of the clamped input against float64); the mean: rule 2 with n = len on sum|log| plus the mean
            of the log bounds and the division; one rounding for the difference.  Inputs 0, 1e-10 and FLT_EPSILON must all give log(FLT_EPSILON).

Bit-identity (the contract at the top of speaker.hip): for the conv, the gate and the pooling every sequence of a batch run alone, at T = its own
length and at T = length + 13, gives the batch's rows bit for bit.

CPU twins (``test_cpu_*``, no gpu mark).  A plain fp32 torch emulation of each kernel (H.spk_*_emulate: the K order of the MFMA steps, the 4-row
group sums, the slice-ordered gate sums, the 4-phase pooling sums, the P-phase CMN sums) runs every GPU case through the same checks and meets
every bound.  test_cpu_injected_faults_miss: each fault misses a bound or leaks a NaN (inf) on a committed case, by the factor printed:
  1 pre_on_pad     prologue applied to padded taps (they contribute relu(shift))          cin = 1 cases with the prologue     5e5 x - 5e6 x
  2 past_len       rows at and past in_len read                                            ragged 3 x 3, TDNN, gated cases     NaN (inf)
  3 no_dilation    time dilation ignored                                                   the dil = 2 gated convs             8e3 x
  4 sf_on_time     the frequency stride applied to time                                    3 x 3, frequency stride 2           1e4 x
  5 gate_shift     gate segment index off by one frame                                     the gated convs, segments of 8      4e4 x - 8e4 x
  6 seg_len        last segment's mean divided by seg_len, not its valid frames           cv_spk_cam_gate, all three cases    5e2 x - 6e2 x
  7 psum_all_rows  psum counts rows >= out_len                                             the psum cases with a ragged length 7e7 x - 1e8 x
  8 biased         std divides by n                                                        cv_spk_stats_pool, all six cases    2e4 x - 1e5 x
  9 mean_T         CMN mean over T rows instead of the length                              cv_spk_log_cmn, cmn = 1             4e6 x

Found by test_spk_stats_pool on MI355X: without the prologue (pre_scale NULL) spk_stats_kernel pooled relu(x) instead of x (9e5 x the bound on
N(0, 1) rows; the model always passes the prologue).  The kernel now applies the ReLU only with the prologue.
"""
import ctypes as C
import functools
import math
import os
import sys
import zlib

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _helpers as H  # noqa: E402

gpu = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
GUARD = 2
NAN = float("nan")


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _tdnn_frames(T):
    return (T - 1) // 2 + 1


# ============================================================================= cv_spk_conv: cases
def _conv_case(B=3, T=9, F_in=1, cin=32, N=32, k=(1, 1), s=(1, 1), pad=(0, 0), dt=1, ldx=None, lens=None, pre=False, bias=False, res=False,
               relu=False, gate_seg=0, psum=False, ldy=None, y_off=0, ragged=True):
    kf, kt = k
    T_out = (T + 2 * pad[1] - dt * (kt - 1) - 1) // s[1] + 1
    F_out = (F_in + 2 * pad[0] - (kf - 1) - 1) // s[0] + 1
    lens = list(lens) if lens is not None else [T, T // 2, 0][:B]
    out_lens = [(_tdnn_frames(n) if s[1] == 2 else n) for n in lens]
    assert T_out == (_tdnn_frames(T) if s[1] == 2 else T)
    return dict(B=B, T_in=T, F_in=F_in, cin=cin, N=N, k=k, s=s, pad=pad, dt=dt, ldx=ldx or (2 if cin == 1 else cin + 4), lens=lens,
                out_lens=out_lens, T_out=T_out, F_out=F_out, pre=pre, bias=bias, res=res, relu=relu, gate_seg=gate_seg, psum=psum,
                ldy=ldy or N + 4, y_off=y_off, ragged=ragged)


CONV_CASES = {}
for _F in (6, 7):                                    # cin = 1: the FCM head's first conv, 3 x 3 pad 1; M = T F = 6 .. 119
    for _T in (1, 9, 17):
        for _pre in (False, True):
            CONV_CASES[f"cin1-F{_F}-T{_T}{'-pre' if _pre else ''}"] = _conv_case(T=_T, F_in=_F, cin=1, k=(3, 3), pad=(1, 1), pre=_pre, bias=True,
                                                                                 relu=True)
# 3 x 3 over (T, F), cin 32: M = T F_out = 64 (exactly one workgroup), 77 and 65 (a second workgroup of 13 / 1 rows), 20 (two waves)
CONV_CASES["c32-sf1-M64-bias-relu"] = _conv_case(T=8, F_in=8, k=(3, 3), pad=(1, 1), bias=True, relu=True)
CONV_CASES["c32-sf1-M77-bias-res-relu"] = _conv_case(T=11, F_in=7, k=(3, 3), pad=(1, 1), bias=True, res=True, relu=True)
CONV_CASES["c32-sf1-M77-bias"] = _conv_case(T=11, F_in=7, k=(3, 3), pad=(1, 1), bias=True)
CONV_CASES["c32-sf2-M65-bias-relu"] = _conv_case(T=13, F_in=10, k=(3, 3), s=(2, 1), pad=(1, 1), bias=True, relu=True)
CONV_CASES["c32-sf2-M65-bias"] = _conv_case(T=13, F_in=10, k=(3, 3), s=(2, 1), pad=(1, 1), bias=True)
CONV_CASES["c32-sf2-M20-bias-res-relu"] = _conv_case(T=4, F_in=9, k=(3, 3), s=(2, 1), pad=(1, 1), bias=True, res=True, relu=True)
for _T in (5, 6, 33):                                # the TDNN: k = (1, 5), time stride 2, pad 2, cin 320, T_out != T_in, out_len != in_len
    CONV_CASES[f"tdnn-T{_T}"] = _conv_case(T=_T, cin=320, N=128, k=(1, 5), s=(1, 2), pad=(0, 2), bias=True, relu=True)
for _cin, _ld in ((128, 512), (160, 1024), (480, 512)):     # dense-block 1 x 1: columns [0, cin) of a wide buffer whose other columns are NaN
    CONV_CASES[f"dense-cin{_cin}-ld{_ld}"] = _conv_case(T=21, cin=_cin, N=128, ldx=_ld, pre=True, bias=True, relu=True, psum=True)
for _T in (1, 3, 4, 5, 63, 64, 65):                  # psum: lengths that end inside a 4-row group
    CONV_CASES[f"psum-T{_T}"] = _conv_case(T=_T, cin=128, N=128, ldx=512, lens=[_T, max(_T - 2, 0), 0], pre=True, bias=True, relu=True, psum=True)
# the CAM layer's local conv: k3, dilation, gated, written at y_off = cin into the wide block buffer
CONV_CASES["gated-dil1-seg8"] = _conv_case(T=21, cin=128, N=32, k=(1, 3), pad=(0, 1), dt=1, gate_seg=8, ldy=512, y_off=160)
CONV_CASES["gated-dil2-seg8"] = _conv_case(T=21, cin=128, N=32, k=(1, 3), pad=(0, 2), dt=2, gate_seg=8, ldy=512, y_off=480)
CONV_CASES["gated-dil2-seg100"] = _conv_case(T=103, cin=128, N=32, k=(1, 3), pad=(0, 2), dt=2, gate_seg=100, ldy=1024, y_off=992)
CONV_CASES["transit-K512"] = _conv_case(T=21, cin=512, N=256, ldx=512, pre=True)
CONV_CASES["last-K1024-N192"] = _conv_case(T=1, cin=1024, N=192, ldx=1024, lens=[1, 1, 1], bias=True, ragged=False)
CONV_IDS = list(CONV_CASES)


@functools.lru_cache(maxsize=None)
def _conv_data(name):
    """Logical operands (CPU fp32): x (B, T_in, F_in, cin) with NaN rows at and past in_len, w (N, kf, kt, cin), pre, bias, res (NaN rows at and
    past out_len), gate (B, segments, N) with NaN segments past out_len."""
    c = CONV_CASES[name]
    g = _gen(name)
    B, T, Fi, cin, N = c["B"], c["T_in"], c["F_in"], c["cin"], c["N"]
    kf, kt = c["k"]
    x = torch.randn(B, T, Fi, cin, generator=g)
    w = torch.randn(N, kf, kt, cin, generator=g) / math.sqrt(kf * kt * cin)
    d = dict(x=x, w=w, pre=None, bias=None, res=None, gate=None)
    if c["pre"]:                                                    # shifts of both signs: relu(shift) != 0 on some channels; cin = 1: + 0.3
        sh = torch.randn(cin, generator=g) * 0.5 if cin > 1 else torch.tensor([0.3])
        d["pre"] = (torch.rand(cin, generator=g) + 0.5, sh)
    if c["bias"]:
        d["bias"] = torch.randn(N, generator=g) * 0.3
    if c["res"]:
        d["res"] = torch.randn(B, c["T_out"], c["F_out"], N, generator=g)
    if c["gate_seg"]:
        d["gate"] = torch.rand(B, (c["T_out"] + c["gate_seg"] - 1) // c["gate_seg"], N, generator=g)
    for b in range(B):
        x[b, c["lens"][b]:] = NAN
        if d["res"] is not None:
            d["res"][b, c["out_lens"][b]:] = NAN
        if d["gate"] is not None:
            d["gate"][b, (c["out_lens"][b] + c["gate_seg"] - 1) // c["gate_seg"]:] = NAN
    d["in_len"], d["out_len"] = torch.tensor(c["lens"]), torch.tensor(c["out_lens"])
    return d


@functools.lru_cache(maxsize=None)
def _conv_expect(name):
    c, d = CONV_CASES[name], _conv_data(name)
    return H.spk_conv_ref64(c, d["x"], d["w"], d["in_len"], d["out_len"], d["pre"], d["bias"], d["res"], d["gate"])


def _conv_checks(who, name, y, psum):
    """y (B, T_out, F_out, N), psum (B, ceil(T_out / 4), N) or None: CPU tensors, whoever made them."""
    ref, bound = _conv_expect(name)
    r = H.check(f"{who} conv {name}", y, ref, bound)[1]
    if CONV_CASES[name]["psum"]:
        pref, pb = H.spk_psum_ref64(y[:, :, 0])
        r = max(r, H.check(f"{who} conv {name} psum", psum, pref, pb)[1])
    return r


def _conv_emulated(name, fault=None):
    c, d = CONV_CASES[name], _conv_data(name)
    return H.spk_conv_emulate(c, d["x"], d["w"], d["in_len"], d["out_len"], d["pre"], d["bias"], d["res"], d["gate"], fault=fault)


def _pack_w(w):
    from cosyvoice_amd.speaker import _pad_k
    return _pad_k(w.reshape(w.shape[0], -1)).contiguous()


def _conv_launch(name, only=None, T_run=None):
    """Run the case on the device from NaN-slacked buffers and check every cell outside the op's window; returns y (B', T_out', F_out, N) and
    psum on the CPU.  only / T_run: sequence ``only`` alone in a batch of one padded (or cut) to T_run input frames."""
    from cosyvoice_amd import _lib as L
    c, d = CONV_CASES[name], _conv_data(name)
    x, res, gate, in_len, out_len = d["x"], d["res"], d["gate"], d["in_len"], d["out_len"]
    T_in, T_out = c["T_in"], c["T_out"]
    if only is not None:
        T_in = T_run
        T_out = _tdnn_frames(T_in) if c["s"][1] == 2 else T_in
        sl = slice(only, only + 1)

        def fit(t, T):          # (1, T', ...) -> (1, T, ...): cut, or padded with NaN rows
            t = t[sl]
            if t.shape[1] >= T:
                return t[:, :T].clone()
            return torch.cat([t, torch.full((1, T - t.shape[1], *t.shape[2:]), NAN)], 1)
        x, in_len, out_len = fit(x, T_in), in_len[sl], out_len[sl]
        res = None if res is None else fit(res, T_out)
        if gate is not None:
            gate = fit(gate, (T_out + c["gate_seg"] - 1) // c["gate_seg"])
    B, Fi, Fo, cin, N, ldx, ldy, y_off = x.shape[0], c["F_in"], c["F_out"], c["cin"], c["N"], c["ldx"], c["ldy"], c["y_off"]
    dev = "cuda"
    xb = H.nan_like((B, T_in + GUARD, Fi, ldx), F32)
    xb[:, :T_in, :, :cin] = x.to(dev)
    yb = H.nan_like((B, T_out + GUARD, Fo, ldy), F32)
    if y_off:                                                       # the block buffer's earlier columns hold data
        yb[..., :y_off] = torch.randn(B, T_out + GUARD, Fo, y_off, generator=_gen(name + "y")).to(dev)
    y0 = yb.clone()
    wd = _pack_w(d["w"]).to(dev)
    p = L.SpkConvParams()
    p.B, p.T_in, p.F_in, p.cin = B, T_in, Fi, cin
    p.x, p.x_bs, p.ldx = xb.data_ptr(), xb.stride(0), ldx
    p.kf, p.kt, p.sf, p.st, p.dt, p.pf, p.pt = c["k"][0], c["k"][1], c["s"][0], c["s"][1], c["dt"], c["pad"][0], c["pad"][1]
    p.w, p.ldw, p.N, p.T_out, p.F_out = wd.data_ptr(), wd.shape[1], N, T_out, Fo
    keep = [xb, yb, wd]
    ro = [("x", xb, xb.clone())]
    if c["ragged"]:
        il, ol = in_len.to(torch.int32).to(dev), out_len.to(torch.int32).to(dev)
        p.in_len, p.out_len = il.data_ptr(), ol.data_ptr()
        keep += [il, ol]
    if d["pre"] is not None:
        sc, sh = d["pre"][0].to(dev), d["pre"][1].to(dev)
        p.pre_scale, p.pre_shift = sc.data_ptr(), sh.data_ptr()
        keep += [sc, sh]
    if d["bias"] is not None:
        bd = d["bias"].to(dev)
        p.bias = bd.data_ptr()
        keep.append(bd)
    if res is not None:
        rb = H.nan_like((B, T_out + GUARD, Fo, N + 8), F32)
        rb[:, :T_out, :, :N] = res.to(dev)
        p.res, p.res_bs, p.ldres = rb.data_ptr(), rb.stride(0), N + 8
        ro.append(("res", rb, rb.clone()))
    if gate is not None:
        nseg = gate.shape[1]
        gb = H.nan_like((B, nseg + 1, N), F32)
        gb[:, :nseg] = gate.to(dev)
        p.gate, p.gate_bs, p.gate_seg = gb.data_ptr(), gb.stride(0), c["gate_seg"]
        ro.append(("gate", gb, gb.clone()))
    G4 = (T_out + 3) // 4
    pb = None
    if c["psum"]:
        pb = H.nan_like((B, G4 + GUARD, N), F32)
        p.psum, p.psum_bs = pb.data_ptr(), pb.stride(0)
    p.relu = int(c["relu"])
    p.y, p.y_bs, p.ldy = yb.data_ptr() + 4 * y_off, yb.stride(0), ldy
    L.check(L.lib().cv_spk_conv(C.byref(p), L.stream_ptr()), "cv_spk_conv")
    torch.cuda.synchronize()
    for nm, buf, before in ro:
        assert torch.equal(H.bits(buf), H.bits(before)), f"{name}: {nm} was modified"
    inside = torch.zeros_like(yb, dtype=torch.bool)
    inside[:, :T_out, :, y_off:y_off + N] = True
    assert torch.equal(H.bits(yb)[~inside], H.bits(y0)[~inside]), f"{name}: a cell outside the output window changed"
    psum = None
    if pb is not None:
        assert bool(torch.isnan(pb[:, G4:]).all()), f"{name}: psum written past its groups"
        psum = pb[:, :G4].cpu()
    return yb[:, :T_out, :, y_off:y_off + N].cpu(), psum


@gpu
@pytest.mark.parametrize("name", CONV_IDS)
def test_spk_conv(name):
    y, psum = _conv_launch(name)
    _conv_checks("MI355X", name, y, psum)


ALONE_CASES = ["cin1-F7-T17-pre", "c32-sf2-M65-bias-relu", "c32-sf1-M77-bias-res-relu", "tdnn-T33", "dense-cin160-ld1024", "psum-T65",
               "gated-dil2-seg8"]


@gpu
@pytest.mark.parametrize("name", ALONE_CASES)
def test_spk_conv_sequence_alone_is_bit_identical(name):
    c = CONV_CASES[name]
    y, psum = _conv_launch(name)
    for b, n in enumerate(c["lens"]):
        if n == 0:
            continue
        for T_run in (n, n + 13):
            ya, pa = _conv_launch(name, only=b, T_run=T_run)
            rows = min(ya.shape[1], y.shape[1])
            assert torch.equal(H.bits(ya[0, :rows]), H.bits(y[b, :rows])), f"{name}: sequence {b} alone at T {T_run} differs"
            assert bool((ya[0, rows:] == 0).all()) and bool((y[b, rows:] == 0).all())
            if psum is not None:
                g = min(pa.shape[1], psum.shape[1])
                assert torch.equal(H.bits(pa[0, :g]), H.bits(psum[b, :g])), f"{name}: psum of sequence {b} alone at T {T_run} differs"


@pytest.mark.parametrize("name", CONV_IDS)
def test_cpu_spk_conv_emulation_meets_bounds(name):
    y, psum = _conv_emulated(name)
    assert _conv_checks("fp32 emulation", name, y, psum) <= 1.0


# ============================================================================= cv_spk_cam_gate
GATE_CASES = {"seg100": (201, 100, [1, 3, 4, 99, 100, 101, 103, 200, 201, 0]), "seg8": (21, 8, [21, 17, 18, 19, 15, 16, 0]),
              "seg4": (9, 4, [9, 5, 6, 7, 8, 0])}


@functools.lru_cache(maxsize=None)
def _gate_data(name):
    T, seg, lens = GATE_CASES[name]
    g = _gen("gate" + name)
    B, G4 = len(lens), (T + 3) // 4
    h = torch.clamp(torch.randn(B, 4 * G4, 128, generator=g) + 0.3, min=0)
    for b, n in enumerate(lens):
        h[b, n:] = 0
    ps = h.reshape(B, G4, 4, 128).sum(2)
    for b, n in enumerate(lens):
        ps[b, (n + 3) // 4:] = NAN                                   # groups past the length are never read
    w1, b1 = torch.randn(64, 128, generator=g) * 0.1, torch.randn(64, generator=g) * 0.1
    w2, b2 = torch.randn(32, 64, generator=g) * 0.3, torch.randn(32, generator=g) * 0.5
    return ps, w1, b1, w2, b2


@functools.lru_cache(maxsize=None)
def _gate_expect(name):
    T, seg, lens = GATE_CASES[name]
    return H.spk_gate_ref64(_gate_data(name)[0], lens, T, seg, *_gate_data(name)[1:])


def _gate_check(who, name, gate):
    ref, bound, e32 = _gate_expect(name)
    return H.check(f"{who} cam_gate {name} (e32 {e32:.2e})", gate, ref, bound)[1]


def _gate_launch(name, only=None, T_run=None):
    from cosyvoice_amd import _lib as L
    T, seg, lens = GATE_CASES[name]
    ps, w1, b1, w2, b2 = _gate_data(name)
    if only is not None:
        T, lens = T_run, [lens[only]]
        G4 = (T + 3) // 4
        ps1 = torch.full((1, G4, 128), NAN)
        k = min(G4, ps.shape[1])
        ps1[0, :k] = ps[only, :k]
        ps = ps1
    B, G4, nseg = len(lens), (T + 3) // 4, (T + seg - 1) // seg
    pb = H.nan_like((B, G4 + GUARD, 128), F32)
    pb[:, :G4] = ps.cuda()
    p0 = pb.clone()
    gb = H.nan_like((B + 1, nseg * 32 + 8), F32)
    ld = torch.tensor(lens, dtype=torch.int32).cuda()
    ws = [t.cuda().contiguous() for t in (w1, b1, w2, b2)]
    L.check(L.lib().cv_spk_cam_gate(C.c_void_p(pb.data_ptr()), C.c_int64(pb.stride(0)), C.c_void_p(ld.data_ptr()), B, T, seg,
                                    *[C.c_void_p(t.data_ptr()) for t in ws], C.c_void_p(gb.data_ptr()), C.c_int64(gb.stride(0)),
                                    L.stream_ptr()), "cv_spk_cam_gate")
    torch.cuda.synchronize()
    assert torch.equal(H.bits(pb), H.bits(p0)), "psum was modified"
    H.window_only(f"cam_gate {name}", gb, B, 0, nseg * 32)
    return gb[:B, :nseg * 32].reshape(B, nseg, 32).cpu()


@gpu
@pytest.mark.parametrize("name", list(GATE_CASES))
def test_spk_cam_gate(name):
    gate = _gate_launch(name)
    _gate_check("MI355X", name, gate)
    T, seg, lens = GATE_CASES[name]
    for b, n in enumerate(lens):
        assert bool((gate[b, (n + seg - 1) // seg:] == 0).all()), "segments past the length must be 0"
        if n == 0:
            continue
        for T_run in (n, n + 13):
            ga = _gate_launch(name, only=b, T_run=T_run)
            k = min(ga.shape[1], gate.shape[1])
            assert torch.equal(H.bits(ga[0, :k]), H.bits(gate[b, :k])), f"sequence {b} alone at T {T_run} differs"


@pytest.mark.parametrize("name", list(GATE_CASES))
def test_cpu_spk_cam_gate_emulation_meets_bounds(name):
    T, seg, lens = GATE_CASES[name]
    assert _gate_check("fp32 emulation", name, H.spk_gate_emulate(_gate_data(name)[0], lens, T, seg, *_gate_data(name)[1:])) <= 1.0


# ============================================================================= cv_spk_stats_pool
POOL_LENS, POOL_T = [2, 3, 4, 5, 131], 131
POOL_CASES = [(Cc, pre) for Cc in (64, 512) for pre in ("none", "bn", "bn+30")]
POOL_IDS = [f"C{Cc}-{pre}" for Cc, pre in POOL_CASES]


@functools.lru_cache(maxsize=None)
def _pool_data(Cc, pre):
    g = _gen(f"pool{Cc}{pre}")
    x = torch.randn(len(POOL_LENS), POOL_T, Cc, generator=g)
    for b, n in enumerate(POOL_LENS):
        x[b, n:] = NAN
    if pre == "none":
        return x, None
    sh = torch.randn(Cc, generator=g) * 0.5 + (30.0 if pre == "bn+30" else 0.0)
    return x, (torch.rand(Cc, generator=g) + 0.5, sh)


@functools.lru_cache(maxsize=None)
def _pool_expect(Cc, pre):
    return H.spk_pool_ref64(*_pool_data(Cc, pre)[:1], POOL_LENS, _pool_data(Cc, pre)[1])


def _pool_check(who, Cc, pre, out):
    ref, bound, e32 = _pool_expect(Cc, pre)
    return H.check(f"{who} stats_pool C {Cc} {pre} (e32 {e32:.2e})", out, ref, bound)[1]


def _pool_launch(Cc, pre, only=None, T_run=None):
    from cosyvoice_amd import _lib as L
    x, pp = _pool_data(Cc, pre)
    lens, T = POOL_LENS, POOL_T
    if only is not None:
        lens, T = [POOL_LENS[only]], T_run
        x1 = torch.full((1, T, Cc), NAN)
        k = min(T, POOL_T)
        x1[0, :k] = x[only, :k]
        x = x1
    B, ldx = len(lens), Cc + 8
    xb = H.nan_like((B, T + GUARD, ldx), F32)
    xb[:, :T, :Cc] = x.cuda()
    x0 = xb.clone()
    ob = H.nan_like((B + 1, 2 * Cc + 8), F32)
    ld = torch.tensor(lens, dtype=torch.int32).cuda()
    sc, sh = (pp[0].cuda(), pp[1].cuda()) if pp is not None else (None, None)
    L.check(L.lib().cv_spk_stats_pool(C.c_void_p(xb.data_ptr()), C.c_int64(xb.stride(0)), ldx, C.c_void_p(ld.data_ptr()), B, T, Cc,
                                      C.c_void_p(L.ptr(sc)), C.c_void_p(L.ptr(sh)), C.c_void_p(ob.data_ptr()), C.c_int64(ob.stride(0)),
                                      L.stream_ptr()), "cv_spk_stats_pool")
    torch.cuda.synchronize()
    assert torch.equal(H.bits(xb), H.bits(x0)), "x was modified"
    H.window_only(f"stats_pool C {Cc}", ob, B, 0, 2 * Cc)
    return ob[:B, :2 * Cc].cpu()


@gpu
@pytest.mark.parametrize("Cc,pre", POOL_CASES, ids=POOL_IDS)
def test_spk_stats_pool(Cc, pre):
    out = _pool_launch(Cc, pre)
    _pool_check("MI355X", Cc, pre, out)
    if Cc == 64:
        for b, n in enumerate(POOL_LENS):
            for T_run in (n, n + 13):
                assert torch.equal(H.bits(_pool_launch(Cc, pre, only=b, T_run=T_run)[0]), H.bits(out[b])), f"sequence {b} alone at T {T_run} differs"


@pytest.mark.parametrize("Cc,pre", POOL_CASES, ids=POOL_IDS)
def test_cpu_spk_stats_pool_emulation_meets_bounds(Cc, pre):
    x, pp = _pool_data(Cc, pre)
    assert _pool_check("fp32 emulation", Cc, pre, H.spk_pool_emulate(x, POOL_LENS, pp)) <= 1.0


# ============================================================================= cv_spk_power
POWER_CASES = [(5, 1), (5, 256), (5, 257), (3, 257)]                # rows nbins = 5, 1280, 1285, 771: the last block is partial in three of them


@functools.lru_cache(maxsize=None)
def _power_data(rows, nbins):
    return torch.randn(rows, 2 * nbins, generator=_gen(f"pow{rows}-{nbins}")) * 30


def _power_check(who, rows, nbins, pw):
    s = _power_data(rows, nbins).double()
    ref = s[:, :nbins] ** 2 + s[:, nbins:] ** 2
    return H.check(f"{who} power rows {rows} nbins {nbins}", pw, ref, H.sum_bound(2, ref, ref, F32))[1]


@gpu
@pytest.mark.parametrize("rows,nbins", POWER_CASES)
def test_spk_power(rows, nbins):
    from cosyvoice_amd import _lib as L
    ld_spec, ld_pow = 2 * nbins + 3, nbins + 5
    sb = H.nan_like((rows + GUARD, ld_spec), F32)
    sb[:rows, :2 * nbins] = _power_data(rows, nbins).cuda()
    s0 = sb.clone()
    pb = H.nan_like((rows + GUARD, ld_pow), F32)
    L.check(L.lib().cv_spk_power(C.c_void_p(sb.data_ptr()), ld_spec, C.c_void_p(pb.data_ptr()), ld_pow, rows, nbins, L.stream_ptr()),
            "cv_spk_power")
    torch.cuda.synchronize()
    assert torch.equal(H.bits(sb), H.bits(s0)), "spec was modified"
    H.window_only("power", pb, rows, 0, nbins)
    _power_check("MI355X", rows, nbins, pb[:rows, :nbins].cpu())


@pytest.mark.parametrize("rows,nbins", POWER_CASES)
def test_cpu_spk_power_emulation_meets_bounds(rows, nbins):
    s = _power_data(rows, nbins)
    assert _power_check("fp32 emulation", rows, nbins, s[:, :nbins] * s[:, :nbins] + s[:, nbins:] * s[:, nbins:]) <= 1.0


# ============================================================================= cv_spk_log_cmn
LOGCMN_T = 50
LOGCMN_LENS = [0, 1, LOGCMN_T]
LOGCMN_CASES = [(nm, cmn) for nm in (1, 23, 80, 256) for cmn in (0, 1)]   # 23: 1024 is no multiple of n_mels (44 phases, 12 idle threads)


@functools.lru_cache(maxsize=None)
def _logcmn_data(nm):
    """mel energies log-uniform over [1e-9, 1e6], with 0, 1e-10 and FLT_EPSILON (the clamp) in rows 0 .. 2 of column 0 of the full-length
    sequence; the one-frame sequence starts with 3.0 (with n_mels = 1 a clamped only value would equal what the clamp makes of the NaN rows behind it)."""
    g = _gen(f"logcmn{nm}")
    mel = torch.exp(torch.rand(len(LOGCMN_LENS), LOGCMN_T, nm, generator=g) * math.log(1e15) + math.log(1e-9))
    for b, n in enumerate(LOGCMN_LENS):
        if n == LOGCMN_T:
            mel[b, 0, 0], mel[b, 1, 0], mel[b, 2, 0] = 0.0, 1e-10, H.FLT_EPSILON
        else:
            mel[b, 0, 0] = 3.0                                       # well above the clamp
        mel[b, n:] = NAN
    return mel


@functools.lru_cache(maxsize=None)
def _logcmn_expect(nm, cmn):
    return H.spk_log_cmn_ref64(_logcmn_data(nm), LOGCMN_LENS, cmn)


def _logcmn_check(who, nm, cmn, out):
    ref, bound, e32 = _logcmn_expect(nm, cmn)
    r = H.check(f"{who} log_cmn n_mels {nm} cmn {cmn} (e32 {e32:.2e})", out, ref, bound)[1]
    if not cmn:                                                      # the clamp: 0, 1e-10 and FLT_EPSILON all give log(FLT_EPSILON), rule 3
        want = torch.full((3,), math.log(H.FLT_EPSILON), dtype=F64)
        H.check(f"{who} log_cmn n_mels {nm} clamp", out[2, :3, 0], want, H.act_bound(torch.tensor(e32), want))
    return r


@gpu
@pytest.mark.parametrize("nm,cmn", LOGCMN_CASES)
def test_spk_log_cmn(nm, cmn):
    from cosyvoice_amd import _lib as L
    B, T = len(LOGCMN_LENS), LOGCMN_T
    ld_mel, ldo = nm + 3, nm + 5
    mb = H.nan_like((B * T + GUARD, ld_mel), F32)
    mb[:B * T, :nm] = _logcmn_data(nm).reshape(B * T, nm).cuda()
    m0 = mb.clone()
    ob = H.nan_like((B * T + GUARD, ldo), F32)
    ld = torch.tensor(LOGCMN_LENS, dtype=torch.int32).cuda()
    L.check(L.lib().cv_spk_log_cmn(C.c_void_p(mb.data_ptr()), ld_mel, C.c_void_p(ld.data_ptr()), B, T, nm, cmn, C.c_void_p(ob.data_ptr()), ldo,
                                   L.stream_ptr()), "cv_spk_log_cmn")
    torch.cuda.synchronize()
    assert torch.equal(H.bits(mb), H.bits(m0)), "mel was modified"
    H.window_only("log_cmn", ob, B * T, 0, nm)
    _logcmn_check("MI355X", nm, cmn, ob[:B * T, :nm].reshape(B, T, nm).cpu())


@pytest.mark.parametrize("nm,cmn", LOGCMN_CASES)
def test_cpu_spk_log_cmn_emulation_meets_bounds(nm, cmn):
    assert _logcmn_check("fp32 emulation", nm, cmn, H.spk_log_cmn_emulate(_logcmn_data(nm), LOGCMN_LENS, cmn)) <= 1.0


# ============================================================================= injected faults
def test_cpu_injected_faults_miss():
    def conv_miss(fault, names):
        out = {}
        for nm in names:
            y, psum = _conv_emulated(nm, fault)
            ref, bound = _conv_expect(nm)
            r = H.worst_ratio(y, ref, bound)
            if CONV_CASES[nm]["psum"]:
                r = max(r, H.worst_ratio(psum, *H.spk_psum_ref64(torch.nan_to_num(y[:, :, 0]))))
            out[nm] = r
        print(f"fault {fault}: misses by", {k: f"{v:.3g}" for k, v in out.items()})
        assert all(v > 1.0 for v in out.values()), (fault, out)
    conv_miss("pre_on_pad", [n for n in CONV_IDS if n.startswith("cin1") and n.endswith("-pre")])
    conv_miss("past_len", [n for n in CONV_IDS if n.startswith(("c32", "tdnn-T33", "cin1-F7-T17", "gated"))])
    conv_miss("no_dilation", ["gated-dil2-seg8", "gated-dil2-seg100"])
    conv_miss("sf_on_time", [n for n in CONV_IDS if n.startswith("c32-sf2")])
    conv_miss("gate_shift", ["gated-dil1-seg8", "gated-dil2-seg8"])
    conv_miss("psum_all_rows", [n for n in CONV_IDS if n.startswith("psum-T") and n != "psum-T1"] + ["dense-cin128-ld512"])
    for name, (T, seg, lens) in GATE_CASES.items():
        r = H.worst_ratio(H.spk_gate_emulate(_gate_data(name)[0], lens, T, seg, *_gate_data(name)[1:], fault="seg_len"), *_gate_expect(name)[:2])
        print(f"fault seg_len: cam_gate {name} misses by {r:.3g}")
        assert r > 1.0
    for Cc, pre in POOL_CASES:
        x, pp = _pool_data(Cc, pre)
        r = H.worst_ratio(H.spk_pool_emulate(x, POOL_LENS, pp, fault="biased"), *_pool_expect(Cc, pre)[:2])
        print(f"fault biased: stats_pool C {Cc} {pre} misses by {r:.3g}")
        assert r > 1.0
    for nm in (1, 23, 80, 256):
        r = H.worst_ratio(H.spk_log_cmn_emulate(_logcmn_data(nm), LOGCMN_LENS, 1, fault="mean_T"), *_logcmn_expect(nm, 1)[:2])
        print(f"fault mean_T: log_cmn n_mels {nm} misses by {r:.3g}")
        assert r > 1.0
