#!/usr/bin/env python3
"""Speaker embedding (Kaldi fbank + CAM++) wall time on one MI355X as a graph replay, against the CPU restatement.

    python tools/speaker_bench.py [--iters 50] [--cpu-threads 16] [--out FILE]

Cases: 1 x {3, 10, 30} s prompts and 8 x 10 s.  GPU: median of ``--iters`` replays of the captured graph (waveform upload
included, embedding download excluded), each timed with events after a warm-up.  CPU: tests/speaker_ref.extract_spk_embedding
(torch fp32 network) at ``--cpu-threads`` threads, median of 3.  Prints one JSON line (and writes it to ``--out``)."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import speaker_ref as R
    from cosyvoice_amd.speaker import CAMPPlus
    from cosyvoice_amd.weights import campplus_state_dict
    sd = campplus_state_dict()
    model = CAMPPlus().load_state_dict(sd)
    res = {"what": "speaker_embedding", "iters": a.iters, "cases": []}
    for B, sec in ((1, 3), (1, 10), (1, 30), (8, 10)):
        waves = [R.test_signal(16000 * sec, seed=i) for i in range(B)]
        arg = waves if B > 1 else waves[0]
        for _ in range(3):
            model.extract_spk_embedding(arg)
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            model.extract_spk_embedding(arg)
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        key = next(k for k in model._graphs if k[0] == "wave" and k[1] == B and k[2] >= 16000 * sec)
        case = {"batch": B, "seconds": sec, "gpu_ms_median": round(statistics.median(ts), 4), "gpu_ms_min": round(min(ts), 4),
                "launches": model.num_launches(key)}
        if B == 1:
            torch.set_num_threads(a.cpu_threads)
            cs = []
            for _ in range(3):
                t0 = time.perf_counter()
                with torch.no_grad():
                    R.extract_spk_embedding(sd, waves[0])
                cs.append((time.perf_counter() - t0) * 1e3)
            case["cpu_ms_median"] = round(statistics.median(cs), 2)
            case["cpu_threads"] = a.cpu_threads
        res["cases"].append(case)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
