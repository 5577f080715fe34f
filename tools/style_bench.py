#!/usr/bin/env python3
"""512-d speaker encoder (cosyvoice_amd/style.py) wall time on one MI355X.

    python tools/style_bench.py [--iters 30] [--cpu-threads 16] [--out profiles/style_bench.json]

Cases: 1 x {3, 10, 30} s prompts and 8 x 10 s at 24 kHz.  Three numbers per case:
  gpu_ms          median of ``--iters`` calls of SpeakerEmbedding (upload, reflect staging, CAM++ graph, noise draw and the replay of the
                  captured graph; the download of the vector excluded), each timed with events after a warm-up;
  posterior_fused_ms / posterior_composed_ms
                  the posterior encoder alone (pre, 16 WaveNet layers, proj) as a captured graph, with one cv_wn_layer per layer
                  against the same layers composed from cv_gemm launches and cv_wn_gate, measured back to back in the same run;
  cpu_ms          tests/style_ref.speaker_embedding (torch fp32) at ``--cpu-threads`` threads, median of 3 (batch 1 only).
Prints one JSON line (and writes it to ``--out``)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _time(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return round(statistics.median(ts), 4), round(min(ts), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import style_ref as R
    from cosyvoice_amd import ops
    from cosyvoice_amd.style import SpeakerEmbedding
    from cosyvoice_amd.weights import speaker_embedding_state_dict
    sd = speaker_embedding_state_dict()
    model = SpeakerEmbedding().load_state_dict(sd)
    gen = torch.Generator(device="cuda").manual_seed(0)
    res = {"what": "speaker_embedding_v2", "iters": a.iters, "cases": []}
    for B, sec in ((1, 3), (1, 10), (1, 30), (8, 10)):
        waves = [R.test_signal(24000 * sec, seed=i) for i in range(B)]
        med, mn = _time(lambda: model(waves, generator=gen), a.iters)
        T = model.bucket(sec * 80)
        case = {"batch": B, "seconds": sec, "frames": sec * 80, "gpu_ms_median": med, "gpu_ms_min": mn, "launches": model.num_launches((B, T))}
        ws = model._ws[(B, T)]
        extra = dict(a=torch.empty(B * T, 1024, device="cuda"), g=torch.empty(B * T, 512, device="cuda"))
        for name, fused in (("posterior_fused_ms", True), ("posterior_composed_ms", False)):
            g = ops.Graph().capture(lambda: model.enc_q.enqueue(ws["mag"], ws["lens"], B, T, ws, fused=fused, extra=extra))
            case[name], case[name[:-3] + "_launches"] = _time(g.launch, a.iters)[0], g.num_launches
            torch.cuda.synchronize()
            g.destroy()
        if B == 1:
            torch.set_num_threads(a.cpu_threads)
            noise = torch.randn(512, sec * 80)
            timbre = torch.randn(192)
            cs = []
            for _ in range(3):
                t0 = time.perf_counter()
                with torch.no_grad():
                    R.speaker_embedding(sd, waves[0], waves[0].numel(), noise, timbre)
                cs.append((time.perf_counter() - t0) * 1e3)
            case["cpu_ms_median"], case["cpu_threads"] = round(statistics.median(cs), 2), a.cpu_threads
        res["cases"].append(case)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
