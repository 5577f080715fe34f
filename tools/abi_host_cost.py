"""Host cost of one call through the ctypes binding, on the CPU (no GPU: the call is rejected before any launch).  cv_decode_attention with
a null q returns CV_ERR_ARG; it is marshalled
  (a) the way call sites did before the prototype table: a bare CDLL function without argtypes, every pointer / float wrapped by hand,
  (b) this tree's way: plain values through the prototype _lib.lib() installed,
  (c) plain values through the same prototype with ctypes' own c_int32 for the 32-bit arguments (why _lib._Int32Arg exists),
the forms alternating, ``--calls`` calls per repeat, ``--repeats`` repeats.  Writes both medians (ns per call) and the spread (max - min
over its repeats) of form (a); acceptance: median(b) <= median(a) + spread(a).

    python tools/abi_host_cost.py [--out profiles/abi_prototypes_host.json] [--calls 300000] [--repeats 7]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cosyvoice_amd import _lib as L  # noqa: E402

PTR = 4096        # a non-null dummy, never dereferenced: q is null, so the entry point returns before it launches anything


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "abi_prototypes_host.json"))
    ap.add_argument("--calls", type=int, default=300000)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    typed = L.lib().cv_decode_attention
    bare = C.CDLL(L.LIB_PATH).cv_decode_attention          # its own function object: no argtypes
    assert bare.argtypes is None and typed.argtypes is not None
    stock = C.CDLL(L.LIB_PATH).cv_decode_attention
    stock.argtypes = [C.c_int32 if t is L._Int32Arg else t for t in typed.argtypes]
    st = C.c_void_p(None)
    vp, f32 = C.c_void_p, C.c_float

    def wrapped(n):
        for _ in range(n):
            bare(vp(None), 896, vp(PTR), vp(PTR), vp(PTR), 1, vp(PTR), 896, 8, 14, 2, 704, f32(0.125), L.CV_F16, vp(None), 0, vp(None), st)

    def plain(n, fn=typed):
        for _ in range(n):
            fn(None, 896, PTR, PTR, PTR, 1, PTR, 896, 8, 14, 2, 704, 0.125, L.CV_F16, None, 0, None, st)

    def plain_c_int32(n):
        plain(n, stock)

    assert bare(vp(None), 896, vp(PTR), vp(PTR), vp(PTR), 1, vp(PTR), 896, 8, 14, 2, 704, f32(0.125), L.CV_F16, vp(None), 0, vp(None), st) == -1
    assert typed(None, 896, PTR, PTR, PTR, 1, PTR, 896, 8, 14, 2, 704, 0.125, L.CV_F16, None, 0, None, st) == -1
    forms = (("wrapped", wrapped), ("plain", plain), ("plain_c_int32", plain_c_int32))
    ns = {name: [] for name, _ in forms}
    for _, fn in forms:
        fn(20000)
    for _ in range(a.repeats):
        for name, fn in forms:
            t0 = time.perf_counter()
            fn(a.calls)
            ns[name].append(round((time.perf_counter() - t0) / a.calls * 1e9, 1))
    med = {k: statistics.median(v) for k, v in ns.items()}
    spread = round(max(ns["wrapped"]) - min(ns["wrapped"]), 1)
    out = {
        "what": "ns per call of cv_decode_attention rejected with CV_ERR_ARG (null q, nothing launched), CPU only, the forms alternating: "
                "'wrapped' = no argtypes, 8 hand-made c_void_p / c_float objects per call (the call sites before the prototype table); "
                "'plain' = plain ints / floats / None through the installed prototype; 'plain_c_int32' = the same call when the prototype's "
                "32-bit arguments are ctypes.c_int32 (an argument object per int) instead of _lib._Int32Arg",
        "calls_per_repeat": a.calls, "repeats": a.repeats, "ns_per_call": ns,
        "wrapped_median_ns": med["wrapped"], "plain_median_ns": med["plain"], "plain_c_int32_median_ns": med["plain_c_int32"],
        "wrapped_spread_ns": spread,
        "acceptance": "plain median <= wrapped median + wrapped spread (max - min over its repeats)",
        "plain_not_above_wrapped_plus_spread": med["plain"] <= med["wrapped"] + spread,
    }
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))
    return 0 if out["plain_not_above_wrapped_plus_spread"] else 1


if __name__ == "__main__":
    sys.exit(main())
