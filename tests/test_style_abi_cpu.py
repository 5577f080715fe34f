"""CPU: the speaker-encoder-v2 entry points (include/cosyvoice_amd_style.h, cosyvoice_amd._lib.STYLE_EXPORTS) — what test_abi_cpu.py
checks for the main header: declarations, exports and the Python list agree, arguments are validated before anything is launched,
and every entry point has a data test."""
import ctypes
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "..", "include", "cosyvoice_amd_style.h")


def _declared():
    return set(re.findall(r"\b(cv_[a-z0-9_]+)\s*\(", open(HEADER).read()))


def test_style_exports_match_header_and_library():
    from cosyvoice_amd import build, _lib
    lib = ctypes.CDLL(build.build(verbose=False))
    declared = _declared()
    assert declared == set(_lib.STYLE_EXPORTS), (sorted(declared - set(_lib.STYLE_EXPORTS)), sorted(set(_lib.STYLE_EXPORTS) - declared))
    assert len(set(_lib.STYLE_EXPORTS)) == len(_lib.STYLE_EXPORTS) and not set(_lib.STYLE_EXPORTS) & set(_lib.EXPORTS)
    for name in _lib.STYLE_EXPORTS:
        assert hasattr(lib, name), f"{name} declared in the header but not exported"
    _lib.style_lib()   # the size handshake of the two parameter blocks


def test_main_header_does_not_declare_style_entry_points():
    from cosyvoice_amd import _lib
    main = open(os.path.join(HERE, "..", "include", "cosyvoice_amd.h")).read()
    for name in _lib.STYLE_EXPORTS:
        assert name not in main


def _wn_block(L):
    p = L.WnLayerParams()
    p.B, p.T, p.C, p.taps, p.n_rs = 1, 32, 512, 5, 1024
    p.len = p.x = p.w_in = p.b_in = p.w_rs = p.b_rs = p.skip = 16
    p.x_out = 32
    p.x_bs = p.xo_bs = p.skip_bs = 32 * 512
    p.ldx = p.ldxo = p.ldskip = 512
    return p


def _glu_block(L):
    p = L.GluConvParams()
    p.B, p.T, p.C, p.taps = 1, 32, 256, 5
    p.len = p.x = p.w = p.bias = 16
    p.y = 32
    p.x_bs = p.y_bs = 32 * 256
    p.ldx = p.ldy = 256
    return p


def test_style_argument_validation_without_a_gpu():
    """Bad arguments come back as a negative cv_status before anything is launched: dummy pointers are never dereferenced.  Each
    block below passes every check until one field is broken."""
    from cosyvoice_amd import _lib as L
    lib = L.style_lib()
    null = ctypes.c_void_p(None)
    ARG, UNSUPPORTED = -1, -3
    assert lib.cv_wn_layer(None, null) == ARG and lib.cv_glu_conv(None, null) == ARG
    for field, bad, want in (("B", 0, ARG), ("T", 0, ARG), ("len", None, ARG), ("x", None, ARG), ("skip", None, ARG), ("C", 256, UNSUPPORTED),
                             ("taps", 3, UNSUPPORTED), ("n_rs", 768, ARG), ("x_out", None, ARG), ("x_out", 16, ARG), ("ldx", 510, ARG),
                             ("ldxo", 256, ARG), ("ldskip", 514, ARG), ("x", 20, ARG), ("B", 70000, ARG)):
        p = _wn_block(L)
        setattr(p, field, bad)
        assert lib.cv_wn_layer(ctypes.byref(p), null) == want, (field, bad)
    for field, bad, want in (("B", -1, ARG), ("T", 0, ARG), ("len", None, ARG), ("w", None, ARG), ("bias", None, ARG), ("y", 16, ARG),
                             ("C", 512, UNSUPPORTED), ("taps", 7, UNSUPPORTED), ("ldy", 255, ARG), ("w", 4, ARG)):
        p = _glu_block(L)
        setattr(p, field, bad)
        assert lib.cv_glu_conv(ctypes.byref(p), null) == want, (field, bad)
    assert lib.cv_wn_gate(None, 1024, 16, 512, 8, 512, null) == ARG and lib.cv_wn_gate(16, 1000, 16, 512, 8, 512, null) == ARG
    f = ctypes.c_float(0.125)
    assert lib.cv_gst_attention(None, 512, 16, 16, 16, 512, 1, 8, 4096, f, null) == ARG
    assert lib.cv_gst_attention(16, 256, 16, 16, 16, 512, 1, 8, 4096, f, null) == ARG          # a query row narrower than 8 heads
    assert lib.cv_gst_attention(16, 512, 16, 16, 16, 512, 1, 8, 0, f, null) == ARG
    assert lib.cv_gst_attention(16, 512, 16, 16, 16, 512, 1, 8, 1 << 20, f, null) == UNSUPPORTED
    assert lib.cv_style_attention(16, 16, 16, 768 * 8, 768, None, 256 * 8, 256, 16, 1, 8, 4, f, null) == ARG
    assert lib.cv_style_attention(16, 16, 16, 768 * 8, 768, 16, 256 * 8, 256, None, 1, 8, 4, f, null) == ARG
    assert lib.cv_style_attention(16, 16, 16, 768 * 8, 770, 16, 256 * 8, 256, 16, 1, 8, 4, f, null) == ARG
    assert lib.cv_style_attention(16, 16, 16, 768 * 2401, 768, 16, 256 * 2401, 256, 16, 1, 2401, 4, f, null) == UNSUPPORTED
    assert lib.cv_posterior_sample(None, 1024, 16, 16, 512, 16, 1, 8, 512, null) == ARG
    assert lib.cv_posterior_sample(16, 512, 16, 16, 512, 16, 1, 8, 512, null) == ARG            # stats rows narrower than [m | logs]
    assert lib.cv_masked_mean(16, 8 * 512, 512, None, 1, 8, 512, 16, 512, null) == ARG
    assert lib.cv_masked_mean(16, 8 * 500, 500, 16, 1, 8, 500, 16, 512, null) == ARG             # C % 64


def test_style_source_has_no_environment_switch():
    src = open(os.path.join(HERE, "..", "cosyvoice_amd", "csrc", "style.hip")).read()
    assert "getenv" not in src


def test_every_style_export_has_a_gpu_test():
    """Every entry point is exercised with data in tests/test_style_gpu.py (by name, or through its wrapper of cosyvoice_amd.style);
    the two sizeof entries are run by whatever binds the library."""
    from cosyvoice_amd import _lib
    text = open(os.path.join(HERE, "test_style_gpu.py")).read()
    for name in _lib.STYLE_EXPORTS:
        if name.startswith("cv_sizeof_"):
            assert name in open(os.path.join(HERE, "..", "cosyvoice_amd", "_lib.py")).read()
            continue
        assert re.search(rf"def test_{name}_|\b{name[3:]}\(", text), f"{name}: tests/test_style_gpu.py has no test of it"
