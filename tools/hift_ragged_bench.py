"""HiFT v2 at B = 8 with utterances of different lengths (seeded, spread over 2 - 12 s of audio): device-event time, warmed, of
  (a) the per-utterance loop of batch-1 `inference` calls with every workspace already cached,
  (b) the same loop when every call meets lengths it has not seen (what a service sees: fresh workspaces + descriptors per length),
  (c) ONE `inference_ragged` call over the padded batch;
and the equal-length decode (B = 8, T = 500: the benchmark's vocoder shape) through this tree's library and — same descriptor,
alternating launch by launch — through another build of the library (--parent-lib: the parent commit's libcosyvoice_amd.so, which reads
the descriptor's prefix it knows), with the parent timed twice per round so that its own run-to-run spread is reported next to the
difference.

    python tools/hift_ragged_bench.py [--parent-lib PATH] [--out profiles/hift_ragged_bench.json] [--reps 10]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cosyvoice_amd import _lib as L, ops  # noqa: E402
from cosyvoice_amd.config import HiftConfig  # noqa: E402
from cosyvoice_amd.hift import HiFTGenerator  # noqa: E402
from cosyvoice_amd.weights import hift_state_dict  # noqa: E402


def timed(fn, reps, warm=2):
    """-> (median device ms, median host ms, all device ms) of fn() over ``reps`` calls after ``warm`` unmeasured ones; fn(i) gets the call index."""
    dev, host = [], []
    for i in range(warm + reps):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn(i)
        e1.record()
        torch.cuda.synchronize()
        if i >= warm:
            dev.append(e0.elapsed_time(e1))
            host.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(dev), statistics.median(host), dev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "hift_ragged_bench.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    cfg = HiftConfig.v2()
    B = 8
    g = torch.Generator().manual_seed(a.seed)
    lens = sorted((torch.randint(100, 601, (B,), generator=g)).tolist(), reverse=True)   # 50 frames per second: 2 - 12 s
    mel = lambda n, s: torch.clamp(torch.randn(1, 80, n, generator=torch.Generator().manual_seed(s)) * 2 - 6, -11.5, 2.0).cuda()
    m = HiFTGenerator(cfg, dtype=torch.float32).load_state_dict(hift_state_dict(cfg))
    zero = torch.zeros(1, 1, 0)
    mels = [mel(n, 10 + i) for i, n in enumerate(lens)]
    T = -(-max(lens) // m.length_bucket) * m.length_bucket
    pad = torch.zeros(B, 80, T, device="cuda")
    for b, x in enumerate(mels):
        pad[b, :, :lens[b]] = x[0]
    res = dict(config="v2", B=B, lengths=lens, padded_frames=T, audio_seconds=sum(lens) / 50.0, reps=a.reps, device=torch.cuda.get_device_name(0))

    def loop_cached(i):
        for x in mels:
            m.inference(x, zero)
    d, h, all_a = timed(loop_cached, a.reps)
    res["a_loop_cached_ms"], res["a_host_ms"] = d, h

    def ragged(i):
        m.inference_ragged(pad, lengths=lens)
    d, h, all_c = timed(ragged, a.reps)
    res["c_ragged_ms"], res["c_host_ms"] = d, h

    # a call whose lengths were never seen: every utterance one frame shorter per call (kernels warm, shapes cold); no warm-up calls by definition
    fresh = [[mel(n - 1 - i, 100 + 10 * i + b) for b, n in enumerate(lens)] for i in range(a.reps)]

    def loop_fresh(i):
        for x in fresh[i]:
            m.inference(x, zero)
    d, h, all_b = timed(loop_fresh, a.reps, warm=0)
    res["b_loop_fresh_lengths_ms"], res["b_host_ms"] = d, h
    res["a_all_ms"], res["b_all_ms"], res["c_all_ms"] = all_a, all_b, all_c

    # ---- equal lengths, B = 8, T = 500: the decode descriptor through this library and the parent's, alternating
    Te = 500
    melE = torch.cat([mel(Te, 50 + b) for b in range(B)])
    m.inference(melE, zero)
    ws = m._ws[(B, Te)]
    desc = ws[("_desc", m.presplit)][0]
    assert not desc.lens
    libs = {"this": L.lib()}
    if a.parent_lib:
        libs["parent"] = C.CDLL(os.path.abspath(a.parent_lib))
        res["parent_lib_gemm_params_bytes"], res["this_lib_gemm_params_bytes"] = libs["parent"].cv_sizeof_gemm_params(), libs["this"].cv_sizeof_gemm_params()

    def one(lib):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        L.check(lib.cv_hift_decode_enqueue(C.byref(desc), L.stream_ptr()), "cv_hift_decode_enqueue")
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)
    order = ["parent", "this", "parent"] if a.parent_lib else ["this", "this"]
    names = ["parent_first", "this", "parent_second"] if a.parent_lib else ["this_first", "this_second"]
    series = {n: [] for n in names}
    for r in range(3 + 2 * a.reps):
        for n, k in zip(names, order):
            t = one(libs[k])
            if r >= 3:
                series[n].append(t)
    eq = {n: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v)) for n, v in series.items()}
    res["equal_length_decode_B8_T500"] = eq
    if a.parent_lib:
        p1, p2, t = eq["parent_first"]["median_ms"], eq["parent_second"]["median_ms"], eq["this"]["median_ms"]
        res["equal_length_parent_vs_itself_pct"] = 100.0 * (p2 - p1) / p1
        res["equal_length_this_vs_parent_pct"] = 100.0 * (t - 0.5 * (p1 + p2)) / (0.5 * (p1 + p2))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if not k.endswith("_all_ms")}))
    ops.close()


if __name__ == "__main__":
    main()
