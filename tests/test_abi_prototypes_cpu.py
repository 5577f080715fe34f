"""CPU: cosyvoice_amd._lib's declarations held to the three headers by the host compiler.  Two generated host-only C++ programs (own
``main``, nothing linked against the library, no GPU) print what the headers say: the class of every export's return type and arguments,
and the offset and size of every struct field.  Both must equal _lib.PROTOTYPES / RETURNS and the ctypes mirrors of _lib.STRUCTS."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
INCLUDE = os.path.join(HERE, "..", "include")


def _header(name):
    return open(os.path.join(INCLUDE, name)).read()


def _run_program(tmp_path, name, body):
    """Compile ``body`` (after the three headers) with the host compiler only and return what it prints."""
    cxx = next((c for c in ("/opt/rocm/llvm/bin/clang++", shutil.which("clang++"), shutil.which("g++")) if c and os.path.exists(c)), None)
    assert cxx, "no host C++ compiler found"
    from cosyvoice_amd import _lib
    src, exe = tmp_path / (name + ".cpp"), tmp_path / name
    src.write_text("#include <cstddef>\n#include <cstdio>\n#include <type_traits>\n"
                   + "".join(f'#include "{h}"\n' for h in _lib.PROTOTYPES) + body)
    r = subprocess.run([cxx, "-std=c++17", "-I", INCLUDE, str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()


SIG = r"""
template <class T> constexpr char cls() {
  if constexpr (std::is_void_v<T>) return 'v';
  else if constexpr (std::is_pointer_v<T>) return 'p';
  else if constexpr (std::is_same_v<T, float>) return 'f';
  else if constexpr (std::is_integral_v<T> || std::is_enum_v<T>) return sizeof(T) == 4 ? 'i' : sizeof(T) == 8 ? 'q' : '?';
  else return '?';
}
template <class R> constexpr char ret() { if constexpr (std::is_same_v<R, const char*>) return 's'; else return cls<R>(); }
template <class F> struct Sig;
template <class R, class... A> struct Sig<R(A...)> {
  static void print(const char* name) { const char args[] = {cls<A>()..., 0}; std::printf("%s %c %s\n", name, ret<R>(), args); }
};
"""


def test_every_prototype_equals_its_header_declaration(tmp_path):
    """decltype(export) through a template that prints one class letter per argument and for the return type (no symbol has to resolve):
    the printed line must be the table's entry, for exactly the names each header declares."""
    from cosyvoice_amd import _lib
    names = [n for table in _lib.PROTOTYPES.values() for n in table]
    assert len(names) == len(set(names)) and set(_lib.RETURNS) <= set(names)
    for header, table in _lib.PROTOTYPES.items():
        declared = set(re.findall(r"\b(cv_[a-z0-9_]+)\s*\(", _header(header)))
        assert declared == set(table), (header, sorted(declared - set(table)), sorted(set(table) - declared))
    assert (_lib.EXPORTS, _lib.STYLE_EXPORTS, _lib.LORA_EXPORTS) == tuple(list(t) for t in _lib.PROTOTYPES.values())
    body = SIG + "int main() {\n" + "".join(f'  Sig<decltype({n})>::print("{n}");\n' for n in names) + "  return 0;\n}\n"
    printed = _run_program(tmp_path, "signatures", body)
    want = [f"{n} {_lib.RETURNS.get(n, 'i')} {sig}" for table in _lib.PROTOTYPES.values() for n, sig in table.items()]
    assert len(printed) == len(want) == len(names)
    for got, exp in zip(printed, want):
        assert got == exp, f"header: {got!r}  _lib: {exp!r}"
        assert "?" not in got and "v" not in got.split(" ", 2)[2], got     # a class the table's letters cannot express


def _header_fields():
    """C struct name -> field names in declaration order, read from the headers' text (comments stripped; every member is a plain
    declarator list).  The generated program binds each struct to exactly that many names, so the compiler confirms the count."""
    text = re.sub(r"/\*.*?\*/", "", "".join(_header(h) for h in ("cosyvoice_amd.h", "cosyvoice_amd_style.h", "cosyvoice_amd_lora.h")), flags=re.S)
    out = {}
    for cname, body in re.findall(r"typedef\s+struct\s+(cv_[a-z0-9_]+)\s*\{([^{}]*)\}", text):
        fields = []
        for stmt in filter(None, (s.strip() for s in body.split(";"))):
            fields += [re.search(r"([A-Za-z_]\w*)\s*(\[\d+\])?$", d.strip()).group(1) for d in stmt.split(",")]
        out[cname] = fields
    return out


def test_every_struct_mirror_has_the_header_layout(tmp_path):
    """offsetof / sizeof of every field named in a mirror's _fields_, and sizeof of the struct, as the host compiler lays the header out;
    the field names and their number must agree as well (a field dropped from a mirror's tail keeps every other offset)."""
    from cosyvoice_amd import _lib
    declared = _header_fields()
    assert len(_lib.STRUCTS) == 26 and {c for _, c, _ in _lib.STRUCTS} == set(declared), set(declared) ^ {c for _, c, _ in _lib.STRUCTS}
    lines = []
    for st, cname, _ in _lib.STRUCTS:
        mine = [f[0] for f in st._fields_]
        assert mine == declared[cname], (cname, "ctypes", mine, "header", declared[cname])
        lines.append(f'  std::printf("{cname} %zu\\n", sizeof({cname}));\n')
        lines.append(f"  {{ static {cname} o; auto& [{', '.join('f%d' % i for i in range(len(mine)))}] = o; }}\n")
        lines += [f'  std::printf("{cname}.{f} %zu %zu\\n", offsetof({cname}, {f}), sizeof((({cname}*)0)->{f}));\n' for f in mine]
    printed = _run_program(tmp_path, "fields", "int main() {\n" + "".join(lines) + "  return 0;\n}\n")
    got = {k: tuple(int(v) for v in rest) for k, *rest in (l.split() for l in printed)}
    n_fields = 0
    for st, cname, _ in _lib.STRUCTS:
        assert got[cname] == (ctypes.sizeof(st),), (cname, got[cname], ctypes.sizeof(st))
        for f, _t in st._fields_:
            d = getattr(st, f)
            assert got[f"{cname}.{f}"] == (d.offset, d.size), (cname, f, "header", got[f"{cname}.{f}"], "ctypes", (d.offset, d.size))
            n_fields += 1
    assert len(got) == n_fields + len(_lib.STRUCTS)


def test_loader_installs_every_prototype_before_it_publishes_the_handle():
    from cosyvoice_amd import _lib as L
    so = L.lib()
    assert L.style_lib() is so is L.lora_lib()
    for name in L.EXPORTS + L.STYLE_EXPORTS + L.LORA_EXPORTS:
        fn = getattr(so, name)
        assert fn.argtypes is not None and fn.restype is not None, name
    assert so.cv_arch() == b"gfx950" and so.cv_groupnorm_workspace_floats(2, 33, 8) == 2 * 8 * 2 * 3
    # a parameter block of the wrong type is an exception in Python, never a call (nothing is launched either way: M = N = K = 0)
    with pytest.raises(ctypes.ArgumentError):
        so.cv_gemm(ctypes.byref(L.AttnParams()), None)
    assert so.cv_gemm(ctypes.byref(L.GemmParams()), None) == -1 and so.cv_gemm(None, None) == -1
    # a 32-bit argument takes an int (or what has __index__), never a float or None; a missing argument raises as well
    for bad in ((1.5, 1, 1), (None, 1, 1), (1, 1)):
        with pytest.raises((ctypes.ArgumentError, TypeError)):
            so.cv_groupnorm_workspace_floats(*bad)
    assert so.cv_groupnorm_workspace_floats(True, 1, 1) == 3
    # every block-taking entry point is typed with its own mirror; the struct table names only exports, each once
    text = "".join(_header(h) for h in L.PROTOTYPES)
    takes = {c: set(re.findall(rf"\b(cv_[a-z0-9_]+)\s*\(\s*const\s+{c}\s*\*", text)) for _, c, _ in L.STRUCTS}
    assert takes == {c: set(entries) for _, c, entries in L.STRUCTS}
    for st, _, entries in L.STRUCTS:
        for e in entries:
            assert getattr(so, e).argtypes[0] is ctypes.POINTER(st), e
