"""CPU: the C-ABI library builds for gfx950, loads, and exports every symbol include/cosyvoice_amd.h declares."""
import ctypes
import os
import re


def test_library_exports_header_symbols():
    from cosyvoice_amd import build, _lib
    path = build.build(verbose=False)
    assert os.path.exists(path)
    lib = ctypes.CDLL(path)
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "cosyvoice_amd.h")).read()
    declared = set(re.findall(r"\b(cv_[a-z0-9_]+)\s*\(", hdr))
    assert declared, "no declarations parsed"
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in the header but not exported"
    lib.cv_arch.restype = ctypes.c_char_p
    assert lib.cv_arch() == b"gfx950"
    _lib.lib()  # struct-size handshake


def test_exports_list_matches_header():
    """cosyvoice_amd._lib.EXPORTS (what the Python side binds) and the header declare the same entry points."""
    from cosyvoice_amd import _lib
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "cosyvoice_amd.h")).read()
    declared = set(re.findall(r"\b(cv_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib.EXPORTS), (sorted(declared - set(_lib.EXPORTS)), sorted(set(_lib.EXPORTS) - declared))


def test_argument_validation_returns_status_codes_without_a_gpu():
    """Error behaviour of the ABI: bad arguments are rejected with a negative cv_status BEFORE anything is launched (so this
    runs on the GPU-less build container), never with an exception or a crash."""
    from cosyvoice_amd import _lib as L
    lib = L.lib()
    null = ctypes.c_void_p(None)
    one = ctypes.c_void_p(16)          # a non-null, 16-byte aligned dummy that is never dereferenced on these paths
    assert lib.cv_gemm(None, null) < 0
    p = L.GemmParams()
    assert lib.cv_gemm(ctypes.byref(p), null) < 0                       # M = N = K = 0
    p.M, p.N, p.K, p.batch, p.dtype = 8, 8, 30, 1, L.CV_BF16            # K not a multiple of the 16-byte chunk
    p.A, p.W, p.out_f32, p.lda, p.ldw, p.ldo32 = 16, 16, 16, 32, 32, 8
    assert lib.cv_gemm(ctypes.byref(p), null) < 0
    p.K, p.dtype = 32, 7                                                 # unknown dtype
    assert lib.cv_gemm(ctypes.byref(p), null) < 0
    assert lib.cv_attention(None, null) < 0
    a = L.AttnParams()
    assert lib.cv_attention(ctypes.byref(a), null) < 0
    assert lib.cv_layernorm(None, null) < 0
    s = L.SkinnyParams()
    assert lib.cv_skinny_gemm(ctypes.byref(s), null) < 0
    s.M, s.N, s.K, s.Wp, s.A, s.lda, s.dtype = 17, 64, 64, 16, 16, 64, L.CV_BF16   # more than 16 rows
    assert lib.cv_skinny_gemm(ctypes.byref(s), null) < 0
    s.M, s.K = 8, 48                                                     # K not a multiple of 32
    assert lib.cv_skinny_gemm(ctypes.byref(s), null) < 0
    assert lib.cv_sample_ras(None, null) < 0
    assert lib.cv_graph_launch(null, null) < 0 and lib.cv_graph_launch_direct(null, null) < 0 and lib.cv_graph_destroy(null) < 0
    assert lib.cv_graph_num_launches(null) < 0
    assert lib.cv_stream_create_cumask(None, 8, None) < 0 and lib.cv_stream_destroy(null) < 0
    assert lib.cv_anti_alias_act(null, null, 0, 1, 1, 1, None, None, None, None, null) < 0
    assert lib.cv_anti_alias_act_cl(one, 4, 0, one, 2, 0, 1, 8, 4, None, None, None, None, null) < 0
    assert lib.cv_stft_magnitude(None, 8, None, 4, 1, 4, ctypes.c_float(1e-9), null) < 0
    assert lib.cv_log_clamp_channels_first(None, 80, None, 1, 1, 80, ctypes.c_float(1e-5), null) < 0
    assert lib.cv_pack_skinny(null, null, 16, 30, 0, null) < 0           # K % 32
    assert lib.cv_decode_attention(null, 0, null, null, None, 1, null, 0, 1, 14, 2, 704, ctypes.c_float(0.125), L.CV_BF16,
                                   None, 0, None, null) < 0
    # pre-split ([8 hi | 8 lo]) outputs need whole groups of 8 channels: C = 12 would put the last group's lo half past the row
    ptrs = (ctypes.c_void_p * 1)(16)
    assert lib.cv_snake_multi(one, 4, 12, 12, 1, ptrs, ptrs, 12, L.CV_F32X3, null) < 0
    assert lib.cv_snake_multi(one, 4, 16, 16, 1, ptrs, ptrs, 12, L.CV_F32X3, null) < 0
    assert lib.cv_tblock_head(None, null) < 0 and lib.cv_tblock_tail(None, null) < 0
    assert lib.cv_hift_decode_enqueue(None, null) < 0


def test_groupnorm_workspace_size_without_a_gpu():
    """cv_groupnorm_workspace_floats: 3 floats (mean and M2 of x - pilot, and the pilot) per (batch, group, 32-row chunk); 0 for empty shapes."""
    from cosyvoice_amd import _lib as L
    f = L.lib().cv_groupnorm_workspace_floats
    f.restype = ctypes.c_int64
    assert f(1, 1, 1) == 3 and f(2, 32, 8) == 2 * 8 * 3 and f(2, 33, 8) == 2 * 8 * 2 * 3 and f(1, 500, 8) == 8 * 16 * 3
    assert f(0, 5, 8) == 0 and f(1, 0, 8) == 0 and f(1, 5, 0) == 0


def _variant_blocks():
    """Parameter blocks that pass every check of their entry point (dummy aligned pointers, never dereferenced: nothing may be launched
    with them), paired with the entry point and the (variant field, out-of-range value) to set."""
    from cosyvoice_amd import _lib as L
    a = L.AttnParams()
    a.dtype, a.B, a.H, a.Hkv, a.Tq, a.Tk = L.CV_BF16, 1, 1, 1, 16, 16
    a.q = a.k = a.vt = a.out = 16
    a.ldq, a.ldk, a.vt_ld, a.ldo, a.scale = 64, 64, 16, 64, 0.125
    t = L.TBlockParams()
    t.dtype, t.R, t.T, t.C, t.inner, t.ff = L.CV_BF16, 1, 16, 256, 512, 1024
    t.x = t.g1 = t.b1n = t.wqkv_p = t.qk = t.vt = 16
    t.ldx, t.eps, t.ldqk, t.vt_ld = 256, 1e-5, 1024, 16
    r = L.ResblockParams()
    r.dtype, r.R, r.T, r.C, r.cin = L.CV_BF16, 1, 16, 256, 256
    r.a = r.w1_p = r.b1 = r.g1 = r.be1 = r.h1 = 16
    r.lda, r.ldh1, r.eps = 256, 256, 1e-5
    g = L.GemmParams()                 # a k = 3 conv on pre-split operands, pre-split activation output
    g.dtype, g.M, g.N, g.K, g.batch, g.cin, g.tap_step, g.x3_flags = L.CV_F32X3, 64, 64, 192, 1, 64, 1, 7
    g.A = g.W = g.out_f32 = g.out_act = 16
    g.lda, g.ldw, g.ldo32, g.ldoa = 64, 192, 64, 64
    return [("cv_attention", a, "mfma", 48), ("cv_attention", a, "waves", 3), ("cv_tblock_head", t, "mt", 5),
            ("cv_resblock_conv1", r, "mt", 5), ("cv_gemm", g, "conv_win", 33)]


def test_out_of_range_variant_fields_are_rejected_without_a_gpu():
    """The kernel-variant fields (cv_attn_params.mfma / waves, cv_tblock_params.mt, cv_resblock_params.mt, cv_gemm_params.conv_win)
    select among tested kernels; a value outside the documented set is CV_ERR_ARG before anything is launched, never silently the
    library's own choice."""
    from cosyvoice_amd import _lib as L
    lib = L.lib()
    null = ctypes.c_void_p(None)
    CV_ERR_ARG = -1
    for entry, p, field, bad in _variant_blocks():
        assert getattr(p, field) == 0
        setattr(p, field, bad)
        assert getattr(lib, entry)(ctypes.byref(p), null) == CV_ERR_ARG, (entry, field, bad)
        setattr(p, field, -1)
        assert getattr(lib, entry)(ctypes.byref(p), null) == CV_ERR_ARG, (entry, field, -1)
        setattr(p, field, 0)


def _flowblock_blocks():
    """cv_tblock_params that pass every check of cv_tblock_head, cv_tblock_tail and cv_tblock_tail_head, and cv_resblock_params that pass those
    of conv1 and conv2 (dummy aligned pointers, never dereferenced: nothing may be launched with them)."""
    from cosyvoice_amd import _lib as L
    t = L.TBlockParams()
    t.dtype, t.R, t.T, t.C, t.inner, t.ff = L.CV_BF16, 1, 16, 256, 512, 1024
    for f in ("x", "g1", "b1n", "wqkv_p", "qk", "vt", "ao", "wo_p", "bo", "g3", "b3n", "w1_p", "bf1", "w2_p", "bf2"):
        setattr(t, f, 16)
    t.ldx, t.eps, t.ldqk, t.vt_ld, t.ldao = 256, 1e-5, 1024, 16, 512
    r = L.ResblockParams()
    r.dtype, r.R, r.T, r.C, r.cin = L.CV_BF16, 1, 16, 256, 256
    for f in ("a", "w1_p", "b1", "g1", "be1", "tadd", "h1", "w2_p", "b2", "g2", "be2", "wr_p", "br", "out"):
        setattr(r, f, 16)
    r.lda, r.ldh1, r.ldo, r.eps = 256, 256, 256, 1e-5
    return t, r


def test_flowblock_argument_contract_without_a_gpu():
    """The row-block kernels' entry points (csrc/flowblock.hip) return CV_ERR_ARG / CV_ERR_UNSUPPORTED for what their kernels cannot take,
    before anything is launched.  Every case changes only the fields named in a block that meets every other check of the entry point, and
    restores them."""
    from cosyvoice_amd import _lib as L
    lib = L.lib()
    null = ctypes.c_void_p(None)
    ARG, UNSUPPORTED = -1, -3          # cv_status of include/cosyvoice_amd.h
    t, r = _flowblock_blocks()
    HEAD, TAIL, BOTH = ("cv_tblock_head",), ("cv_tblock_tail",), ("cv_tblock_tail_head",)
    RES = ("cv_resblock_conv1", "cv_resblock_conv2")
    cases = [   # (block, entry points, {field: bad value}, status)
        (t, HEAD + BOTH, dict(ldqk=1028), ARG),                    # ldqk % 8: [Q | K] rows are written with 16-byte stores
        (t, HEAD + BOTH, dict(vt_ld=18), ARG),                     # vt_ld % 4
        (t, HEAD + BOTH, dict(T=17, vt_ld=16), ARG),               # vt_ld < T
        (t, HEAD + BOTH, dict(qk=24), ARG),                        # qk not 16-byte aligned
        (t, HEAD + TAIL + BOTH, dict(x=24), ARG),                  # x not 16-byte aligned
        (t, HEAD + TAIL + BOTH, dict(ldx=258), ARG),               # ldx % 4
        (t, BOTH, dict(out_act=16, ldoa=256), ARG),                # the 16-bit copy belongs to a block without a following head
        (t, TAIL + BOTH, dict(wo_p=0), ARG),                       # ao without wo_p
        (t, HEAD + BOTH, dict(T=1 << 20, vt_ld=1 << 20, ldqk=1024), ARG),   # T ldqk 2 = 2^31: past the 32-bit buffer offsets
        (t, HEAD + TAIL + BOTH, dict(C=128), UNSUPPORTED), (t, HEAD + TAIL + BOTH, dict(inner=256), UNSUPPORTED),
        (t, HEAD + TAIL + BOTH, dict(ff=2048), UNSUPPORTED), (t, HEAD + TAIL + BOTH, dict(dtype=L.CV_F32), UNSUPPORTED),
        (r, RES, dict(cin=320, lda=312), ARG),                     # lda < cin
        (r, RES, dict(lda=260), ARG),                              # lda % 8
        (r, RES, dict(cin=384, lda=384), UNSUPPORTED), (r, RES, dict(dtype=L.CV_F32), UNSUPPORTED),
    ]
    for blk, entries, bad, status in cases:
        saved = {f: getattr(blk, f) for f in bad}
        for f, v in bad.items():
            setattr(blk, f, v)
        for e in entries:
            assert getattr(lib, e)(ctypes.byref(blk), null) == status, (e, bad, status)
        for f, v in saved.items():
            setattr(blk, f, v)


def test_csrc_reads_no_environment_variable():
    """Kernel variants are chosen by fields of a call's own parameter block: no source of the library calls getenv."""
    csrc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "cosyvoice_amd", "csrc")
    files = sorted(f for f in os.listdir(csrc) if f.endswith((".hip", ".h")))
    assert len(files) >= 10, files
    for f in files:
        assert "getenv" not in open(os.path.join(csrc, f)).read(), f


def test_version_and_unbound_entry_points_reject_null_arguments():
    """cv_version, and the entry points no Python wrapper calls (aliases of cv_graph_launch / cv_graph_destroy / cv_hift_decode_enqueue, and
    the *_enqueue forms of the composed stages): they answer, and reject null descriptors / handles with a status code."""
    from cosyvoice_amd import _lib as L
    lib = L.lib()
    null = ctypes.c_void_p(None)
    assert lib.cv_version() >= 1
    assert lib.cv_llm_step_enqueue(None, null) < 0 and lib.cv_flow_euler_enqueue(None, null) < 0 and lib.cv_hift_decode(None, null) < 0
    assert lib.cv_llm_step_graph_launch(null, null) < 0 and lib.cv_llm_step_graph_destroy(null) < 0
    assert lib.cv_flow_euler_graph_launch(null, null) < 0 and lib.cv_flow_euler_graph_destroy(null) < 0
    assert lib.cv_hift_decode_graph_create(None, null, None) < 0 and lib.cv_graph_end(null, None) < 0


# Where every entry point of the C ABI is exercised WITH DATA: export -> test module, or (test module, the token in that module that reaches
# it when neither the export's name nor ``ops.<name without cv_>`` appears there).  "lifecycle": create / destroy / sizeof entries, run by
# every test that loads the library or builds a model.  "test_abi_cpu": answered / rejected with null arguments only — these have no data
# test of their own (aliases of tested entry points, and the eager *_enqueue forms of stages that the tests run through *_graph_create).
# A new export fails test_every_export_has_a_test_module until somebody decides where it is tested.
_HELPERS, _GRAPH = "test_helper_kernels_gpu", ("test_flow_gpu", "use_graph = True")
_LLM_OPS = "test_llm_ops_gpu"
_FLOWBLOCK = "test_flowblock_ops_gpu"
_SPK_OPS, _NORM_ACT = "test_speaker_ops_gpu", "test_norm_act_ops_gpu"
COVERAGE = {
    "cv_version": "test_abi_cpu", "cv_arch": "test_abi_cpu",
    "cv_gemm": "test_gemm_modes_gpu", "cv_layernorm": "test_gemm_gpu", "cv_attention": "test_attention_ops_gpu",
    "cv_sizeof_gemm_params": "lifecycle", "cv_sizeof_norm_params": "lifecycle", "cv_sizeof_attn_params": "lifecycle",
    "cv_to_channels_last": _HELPERS, "cv_to_channels_first": _HELPERS, "cv_snake_multi": _HELPERS, "cv_stft16": _HELPERS,
    "cv_istft16": _HELPERS, "cv_hift_source": _HELPERS, "cv_embedding": _HELPERS, "cv_est_pack": _HELPERS, "cv_cfm_update": _HELPERS,
    "cv_graph_begin": _GRAPH, "cv_graph_end": _GRAPH, "cv_graph_launch": _GRAPH, "cv_graph_destroy": "lifecycle",
    "cv_graph_launch_direct": ("test_model_gpu", "cu_partition"), "cv_graph_num_launches": ("test_speaker_gpu", "num_launches"),
    "cv_stream_create_cumask": ("test_model_gpu", "cu_partition"), "cv_stream_destroy": "lifecycle",
    "cv_skinny_gemm": _LLM_OPS, "cv_pack_skinny": _LLM_OPS, "cv_rmsnorm_reduce": _LLM_OPS, "cv_rope_append": _LLM_OPS,
    "cv_decode_attention": _LLM_OPS, "cv_kv_retile": _LLM_OPS, "cv_sample_ras": "test_llm_gpu",
    "cv_sizeof_skinny_params": "lifecycle", "cv_sizeof_sample_params": "lifecycle",
    "cv_anti_alias_act": _NORM_ACT, "cv_anti_alias_act_cl": _NORM_ACT,
    "cv_stft_magnitude": _HELPERS, "cv_log_clamp_channels_first": _HELPERS,
    "cv_groupnorm_cl": _NORM_ACT, "cv_groupnorm_workspace_floats": (_NORM_ACT, "ops.groupnorm_workspace"),
    "cv_interp_linear_cl": _HELPERS, "cv_sizeof_groupnorm_params": "lifecycle", "cv_relpos_append": _HELPERS,
    "cv_sizeof_tblock_params": "lifecycle", "cv_tblock_head": _FLOWBLOCK, "cv_tblock_tail": _FLOWBLOCK,
    "cv_tblock_tail_head": _FLOWBLOCK,
    "cv_sizeof_llm_step_desc": "lifecycle", "cv_sizeof_llm_layer": "lifecycle", "cv_llm_step_enqueue": "test_abi_cpu",
    "cv_llm_step_graph_create": "test_llm_gpu", "cv_llm_step_graph_launch": "test_abi_cpu", "cv_llm_step_graph_destroy": "lifecycle",
    "cv_sizeof_resblock_params": "lifecycle", "cv_resblock_conv1": _FLOWBLOCK, "cv_resblock_conv2": _FLOWBLOCK,
    "cv_sizeof_flow_solver_desc": "lifecycle", "cv_sizeof_flow_block": "lifecycle", "cv_sizeof_flow_tblock": "lifecycle",
    "cv_flow_euler_enqueue": "test_abi_cpu", "cv_flow_euler_graph_create": "test_tblock_gpu", "cv_flow_euler_graph_launch": "test_abi_cpu",
    "cv_flow_euler_graph_destroy": "lifecycle",
    "cv_sizeof_hift_decode_desc": "lifecycle", "cv_sizeof_hift_stage": "lifecycle", "cv_sizeof_hift_resunit": "lifecycle",
    "cv_hift_decode_enqueue": "test_hift_gpu", "cv_hift_decode": "test_abi_cpu", "cv_hift_decode_graph_create": "lifecycle",
    "cv_spk_power": _SPK_OPS, "cv_spk_log_cmn": _SPK_OPS, "cv_sizeof_spk_conv_params": "lifecycle",
    "cv_spk_conv": _SPK_OPS, "cv_spk_cam_gate": _SPK_OPS, "cv_spk_stats_pool": _SPK_OPS,
}


def test_every_export_has_a_test_module():
    from cosyvoice_amd import _lib
    assert set(COVERAGE) == set(_lib.EXPORTS), (sorted(set(_lib.EXPORTS) - set(COVERAGE)), sorted(set(COVERAGE) - set(_lib.EXPORTS)))
    here = os.path.dirname(os.path.abspath(__file__))
    for name, where in COVERAGE.items():
        if where == "lifecycle":
            assert re.search(r"sizeof|create|destroy", name), f"{name} is not a create / destroy / sizeof entry"
            continue
        module, token = where if isinstance(where, tuple) else (where, None)
        path = os.path.join(here, module + ".py")
        assert os.path.exists(path), f"{name}: {module}.py does not exist"
        text = open(path).read()
        pat = re.escape(token) if token else rf"\b{name}\b|\bops\.{name[3:]}\b"
        assert re.search(pat, text), f"{name}: tests/{module}.py names neither it nor its ops wrapper"
