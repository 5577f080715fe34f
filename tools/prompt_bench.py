#!/usr/bin/env python3
"""Prompt front end (resample 16 -> 24 kHz, ragged mel, Kaldi fbank + CAM++, dict assembly) on one MI355X, against the CPU
restatement of the same chain.

    python tools/prompt_bench.py [--iters 20] [--cpu-threads 16] [--out profiles/prompt_frontend_bench.json]

Cases: 1 x {3, 10, 30} s prompts and 8 x 10 s.  GPU: ``PromptFrontEnd.batch`` (waveform upload included), device time between two
events, median of ``--iters`` (>= 10) calls after 3 warm-up calls.  CPU: tests/prompt_ref.prompt_feat + the 24 kHz trim +
tests/speaker_ref.extract_spk_embedding per prompt at ``--cpu-threads`` threads, median of 3.  No threshold: the JSON line (printed
and written to ``--out``) is the record."""
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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prompt_frontend_bench.json"))
    a = ap.parse_args()
    iters = max(10, a.iters)
    import prompt_ref as P
    import speaker_ref as R
    from cosyvoice_amd.frontend import MelSpectrogram, PromptFrontEnd, slaney_mel_basis
    from cosyvoice_amd.speaker import CAMPPlus
    from cosyvoice_amd.weights import campplus_state_dict
    sd = campplus_state_dict()
    fe = PromptFrontEnd(MelSpectrogram(), CAMPPlus().load_state_dict(sd))
    basis = torch.from_numpy(slaney_mel_basis(24000, 1920, 80, 0, 8000))
    g = torch.Generator().manual_seed(0)
    res = {"what": "prompt_frontend", "iters": iters, "warmup": 3, "cases": []}
    for B, sec in ((1, 3), (1, 10), (1, 30), (8, 10)):
        waves = [R.test_signal(16000 * sec, seed=i) for i in range(B)]
        toks = [torch.randint(0, 6561, (25 * sec,), generator=g, dtype=torch.int32) for _ in range(B)]
        texts = [torch.randint(0, 1000, (1, 20), generator=g, dtype=torch.int32) for _ in range(B)]
        for _ in range(3):
            fe.batch(texts, texts, waves, toks)
        torch.cuda.synchronize()
        ts = []
        for _ in range(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            d = fe.batch(texts, texts, waves, toks)
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        case = {"batch": B, "seconds": sec, "gpu_ms_median": round(statistics.median(ts), 4), "gpu_ms_min": round(min(ts), 4),
                "prompt_frames": int(d["prompt_speech_feats"].shape[1])}
        torch.set_num_threads(a.cpu_threads)
        cs = []
        for _ in range(3):
            t0 = time.perf_counter()
            with torch.no_grad():
                for w, t in zip(waves, toks):
                    feat = P.prompt_feat(w, 24000, basis)
                    P.zero_shot(texts[0], texts[0], feat, t[None], R.extract_spk_embedding(sd, w), 24000)
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
