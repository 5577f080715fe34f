"""CPU: what cv_skinny_gemm and cv_attention pick, held to a recording of what they picked before the selection became its own function.

csrc/skinny_select.h and csrc/attn_select.h are plain C++ over the public header: a host-only program (own ``main``, no HIP, nothing linked
against the library) runs them over the inputs of tests/golden/skinny_select.json and must print, for every entry, the recorded status,
kernel form, grid, block and dynamic LDS bytes — and the ksplit / max_wgs (q_hs / k_hs) the kernel is then passed.  The golden was
recorded from the former launch code itself with the launch replaced by a recorder of the stringified kernel expression."""
import json
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")

# Text driver: one line per case, ``skinny k=v ...`` or ``attn k=v ...``; every field not named keeps the default set below.  Pointer
# fields take 0 (null), 1 / 2 (two distinct 64-byte-aligned addresses; nothing is dereferenced), 3 (misaligned).
DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include "cosyvoice_amd/csrc/skinny_select.h"
#include "cosyvoice_amd/csrc/attn_select.h"

static char g_mem[64] __attribute__((aligned(64)));
typedef std::map<std::string, long long> KV;
static long long get(const KV& kv, const char* k, long long d) { auto it = kv.find(k); return it == kv.end() ? d : it->second; }
template <class T> static T* ptr(const KV& kv, const char* k, long long d) {
  const long long v = get(kv, k, d);
  return v == 0 ? nullptr : (T*)(g_mem + (v == 1 ? 0 : (v == 2 ? 16 : 1)));
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream is(line);
    std::string kind, tok;
    is >> kind;
    KV kv;
    while (is >> tok) { const size_t e = tok.find('='); kv[tok.substr(0, e)] = atoll(tok.c_str() + e + 1); }
    if (kind == "skinny") {
      cv_skinny_params p;
      memset(&p, 0, sizeof p);
      p.dtype = (int32_t)get(kv, "dtype", CV_BF16); p.M = (int32_t)get(kv, "M", 1); p.N = (int32_t)get(kv, "N", 896); p.K = (int32_t)get(kv, "K", 896);
      p.A = ptr<void>(kv, "A", 1); p.lda = (int32_t)get(kv, "lda", p.K); p.Wp = ptr<void>(kv, "Wp", 1);
      p.ksplit = (int32_t)get(kv, "ksplit", 1); p.mode = (int32_t)get(kv, "mode", 0);
      p.out_f32 = ptr<float>(kv, "out_f32", 1); p.ldo = p.N; p.out_act = ptr<void>(kv, "out_act", 1); p.ldoa = (int32_t)get(kv, "ldoa", p.N);
      p.nx = ptr<float>(kv, "nx", 1); p.ldnx = (int32_t)get(kv, "ldnx", p.K);
      p.nslabs = ptr<float>(kv, "nslabs", 1); p.n_nslab = (int32_t)get(kv, "n_nslab", 0);
      p.nslab_stride = get(kv, "nslab_stride", 16 * (long long)p.K); p.ld_nslab = (int32_t)get(kv, "ld_nslab", p.K);
      p.ngamma = ptr<float>(kv, "ngamma", 0); p.nx_out = ptr<float>(kv, "nx_out", 0);
      p.max_wgs = (int32_t)get(kv, "max_wgs", 0);
      p.xb_out = ptr<void>(kv, "xb_out", 0); p.ldxb = (int32_t)get(kv, "ldxb", p.N); p.ss_part = ptr<float>(kv, "ss_part", 0);
      p.rs_part = ptr<float>(kv, "rs_part", 0); p.n_rs_part = (int32_t)get(kv, "n_rs_part", 56);
      SkinnySel s;
      // cv_skinny_gemm: null block, then the selector, then the element type (llm.hip)
      int rc = get(kv, "null", 0) ? CV_ERR_ARG : skinny_select(p, &s);
      if (rc == CV_OK && p.dtype != CV_BF16 && p.dtype != CV_F16) rc = CV_ERR_UNSUPPORTED;
      if (rc != CV_OK) { printf("%d\n", rc); continue; }
      printf("%d %d %d %d %d %d %d %d %d %d %u %u 1 256 %zu %d %d\n", rc, (int)skinny_built(s.stream, s.tpw, s.norm, s.tpr, s.u, s.rs, s.mr),
             (int)s.stream, s.tpw, s.norm, s.tpr, s.u, (int)s.rs, s.mr, p.dtype, s.grid_x, s.grid_y, s.lds, p.ksplit, p.max_wgs);
    } else if (kind == "attn") {
      cv_attn_params p;
      memset(&p, 0, sizeof p);
      p.dtype = (int32_t)get(kv, "dtype", CV_BF16); p.B = (int32_t)get(kv, "B", 1); p.H = (int32_t)get(kv, "H", 8); p.Hkv = (int32_t)get(kv, "Hkv", p.H);
      p.Tq = (int32_t)get(kv, "Tq", 100); p.Tk = (int32_t)get(kv, "Tk", p.Tq);
      p.q = ptr<void>(kv, "q", 1); p.k = ptr<void>(kv, "k", 1); p.vt = ptr<void>(kv, "vt", 1); p.out = ptr<void>(kv, "out", 1);
      p.ldq = (int32_t)get(kv, "ldq", 512); p.ldk = (int32_t)get(kv, "ldk", 512); p.vt_ld = (int32_t)get(kv, "vt_ld", (p.Tk + 7) & ~7); p.ldo = (int32_t)get(kv, "ldo", 512);
      p.q_bs = get(kv, "q_bs", 512ll * p.Tq); p.k_bs = get(kv, "k_bs", 512ll * p.Tk); p.o_bs = get(kv, "o_bs", 512ll * p.Tq);
      p.q_hs = get(kv, "q_hs", 0); p.k_hs = get(kv, "k_hs", 0); p.q_off = (int32_t)get(kv, "q_off", 0);
      p.bias = ptr<float>(kv, "bias", 0); p.mfma = (int32_t)get(kv, "mfma", 0); p.waves = (int32_t)get(kv, "waves", 0);
      AttnSel s;
      const int rc = get(kv, "null", 0) ? CV_ERR_ARG : attn_select(p, &s);
      if (rc != CV_OK) { printf("%d\n", rc); continue; }
      printf("%d %d %d %d %u %u %u %u %zu %lld %lld\n", rc, s.form, s.waves, p.dtype, s.grid_x, s.grid_y, s.grid_z, s.block, s.lds,
             (long long)p.q_hs, (long long)p.k_hs);
    }
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(HERE, "golden", "skinny_select.json")))


@pytest.fixture(scope="module")
def select(tmp_path_factory):
    """Compile the driver with the host compiler only; returns run(lines) -> one list of ints per line."""
    cxx = next((c for c in ("/opt/rocm/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++")) if c and os.path.exists(c)), None)
    assert cxx, "no host C++ compiler found"
    d = tmp_path_factory.mktemp("select")
    src, exe = d / "select.cpp", d / "select"
    src.write_text(DRIVER)
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", ROOT, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]

    def run(lines):
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(lines)
        return [[int(x) for x in o.split()] for o in out]
    return run


def skinny_form(kernel):
    """'(skinny_kernel<DT, 2, 0, 16, 7, true, 2>)' -> (stream, TPW, NORM, TPR, U, RS, MR) with the templates' defaults filled in."""
    m = re.fullmatch(r"\((skinny_kernel|skinny_stream_kernel)<DT, ([^>]*)>\)", kernel)
    a = [x.strip() for x in m.group(2).split(",")]
    val = lambda x: 1 if x == "true" else (0 if x == "false" else int(x))
    if m.group(1) == "skinny_stream_kernel":
        assert len(a) == 5 and a[4] == "true"           # the former LOOP argument, only ever true
        return (1, *map(int, a[:4]), 0, 1)
    a = [val(x) for x in a] + [0, 1][len(a) - 4:]
    assert len(a) == 6
    return (0, *a)


def skinny_lines(golden):
    sw = golden["skinny_sweep"]
    lines, want = [], []
    for si, M, mode, nn, flag, ks, mw, status, *rest in sw["rows"]:
        N, K = sw["shapes"][si]
        s = f"skinny M={M} N={N} K={K} mode={mode} ksplit={ks} max_wgs={mw}"
        if nn >= 0:
            s += f" ngamma=1 n_nslab={nn} nx_out=2"
        if flag and mode == 2:
            s += " rs_part=1"
        if flag and mode == 1:
            s += " xb_out=1 ss_part=1"
        lines.append(s)
        if rest:
            kernel, gx, gy, lds, ksplit, max_wgs = rest
            want.append([status, sw["kernels"][kernel], 1, gx, gy, 1, 256, lds, ksplit, max_wgs])
        else:
            want.append([status])
    for line, res in golden["skinny_cases"]:
        lines.append(line)
        want.append(res)
    return lines, want


def test_skinny_select_picks_what_the_former_launch_code_picked(golden, select):
    lines, want = skinny_lines(golden)
    assert len(lines) > 1700
    got = select(lines)
    for line, g, w in zip(lines, got, want):
        if len(w) == 1:
            assert g == w, (line, g, w)
            continue
        status, kernel, dtype, gx, gy, gz, block, lds, ksplit, max_wgs = w
        assert g[0] == status == 0 and g[1] == 1, (line, g, w)            # accepted, and a form the library builds
        assert tuple(g[2:9]) == skinny_form(kernel), (line, g, w)
        assert g[9:] == [dtype, gx, gy, gz, block, lds, ksplit, max_wgs], (line, g, w)


def test_golden_reaches_every_built_form_and_every_status(golden):
    """82 forms per element type: 54 single-shot + 28 streaming.  The recording reaches each one, and each of the three status codes."""
    _, want = skinny_lines(golden)
    forms = {skinny_form(w[1]) for w in want if len(w) > 1}
    assert len(forms) == 82 and sum(1 for f in forms if f[0]) == 28
    assert {w[0] for w in want} == {0, -1, -3}
    assert {w[2] for w in want if len(w) > 1} == {1, 2}                   # bf16 and fp16


def test_skinny_built_is_exactly_the_recorded_set(golden, select, tmp_path):
    """skinny_built (the one statement of which forms exist) over the whole cross product of its arguments' values."""
    _, want = skinny_lines(golden)
    forms = {skinny_form(w[1]) for w in want if len(w) > 1}
    cxx = next((c for c in ("/opt/rocm/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++")) if c and os.path.exists(c)), None)
    src, exe = tmp_path / "built.cpp", tmp_path / "built"
    src.write_text('#include <cstdio>\n#include "cosyvoice_amd/csrc/skinny_select.h"\nint main() {\n'
                   "  const int tpw[] = {0, 1, 2, 3, 4}, nm[] = {0, 1, 2, 3, 4, 5, 6}, tpr[] = {8, 16, 32, 64, 128}, u[] = {4, 6, 7, 8, 9, 10, 12, 14, 16, 20};\n"
                   "  for (int st = 0; st < 2; ++st) for (int a : tpw) for (int b : nm) for (int c : tpr) for (int d : u) for (int rs = 0; rs < 2; ++rs)\n"
                   "    for (int mr = 0; mr < 4; ++mr) if (skinny_built(st, a, b, c, d, rs, mr)) printf(\"%d %d %d %d %d %d %d\\n\", st, a, b, c, d, rs, mr);\n"
                   "  return 0;\n}\n")
    r = subprocess.run([cxx, "-std=c++17", "-I", ROOT, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    built = {tuple(int(x) for x in l.split()) for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()}
    assert built == forms, (sorted(built - forms), sorted(forms - built))


def test_attn_select_picks_what_the_former_launch_code_picked(golden, select):
    sw = golden["attn_sweep"]
    cases = [(f"attn {sw['geometries'][g]} mfma={mf} waves={wv} bias={bias}", [status, sw["kernels"][k], *rest, 64, 64])
             for g, mf, wv, bias, status, k, *rest in sw["rows"]] + [tuple(c) for c in golden["attn_cases"]]
    assert len(cases) > 390
    got = select([line for line, _ in cases])
    seen = set()
    for (line, w), g in zip(cases, got):
        if len(w) == 1:
            assert g == w, (line, g, w)
            continue
        status, kernel, dtype, gx, gy, gz, block, lds, q_hs, k_hs = w
        m = re.fullmatch(r"\((attn_kernel|attn32_kernel|attn64_kernel)<(CV_BF16|CV_F16)(?:, (\d))?>\)", kernel)
        form = {"attn_kernel": 16, "attn32_kernel": 32, "attn64_kernel": 64}[m.group(1)]
        waves = int(m.group(3)) if m.group(3) else 4
        assert {"CV_BF16": 1, "CV_F16": 2}[m.group(2)] == dtype
        assert g == [status, form, waves, dtype, gx, gy, gz, block, lds, q_hs, k_hs], (line, g, w)
        assert block == 64 * waves
        seen.add((form, waves))
    assert seen == {(16, 2), (16, 4), (32, 2), (32, 4), (64, 4)}
    assert {w[0] for _, w in cases} == {0, -1, -3}
