"""What per-sequence LoRA costs the LLM stage: full-size synthetic weights, fp16, the bench's request shape (prefill 282 rows per sequence,
forced tokens), rank 16.  Decode step at 8 and 32 rows and the prefill at 8 x 282 rows, four variants:

  (a) today's graph, adapters=None                 the baseline
  (b) LoRA step, every row -1                      the cost of un-fusing alone (split form + the extra launches, no adapter traffic)
  (c) LoRA step, one adapter shared by all rows    adapter traffic served from L2
  (d) LoRA step, every row a distinct adapter      worst-case adapter streaming (17.6 MB per distinct adapter and step)

A step time is (time of 1 + N steps - time of 1 step) / N of generate_batch, host clock around a device synchronise, graph replays on all
CUs; the variants alternate inside every round and the median over the rounds is reported with the spread.  Run under `timeout`:
    timeout 900 python tools/lora_bench.py [--out profiles/lora_bench.json] [--steps 128] [--rounds 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench as B  # noqa: E402
from cosyvoice_amd.config import FlowConfig, LlmConfig  # noqa: E402
from cosyvoice_amd.llm import Qwen2LM  # noqa: E402
from cosyvoice_amd.lora import LoraBank  # noqa: E402
from cosyvoice_amd.weights import llm_lora_state_dict, llm_state_dict  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "lora_bench.json"))
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rank", type=int, default=16)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lora_bench needs the GPU: nothing is measured without one")
    lc, fc = LlmConfig.full(), FlowConfig.full()
    dt, dev, rows_max = torch.float16, "cuda", 32
    llm = Qwen2LM(lc, dtype=dt, max_batch=rows_max, ctx_max=704, max_out=258).load_state_dict(llm_state_dict(lc))
    bank = LoraBank(llm, max_adapters=rows_max, r=args.rank)
    sd = llm_lora_state_dict(lc, r=args.rank)
    for i in range(rows_max):          # equal contents in distinct memory: the traffic of distinct adapters
        bank.add(f"voice{i}", sd)
    llm.attach_lora(bank)
    texts, forced, ptext, pspeech, _, _ = B.make_inputs(lc, fc, 100, n_utts=rows_max)
    texts = [t.to(dev) for t in texts]
    pt, ps = ptext.to(dev), pspeech.to(dev)
    n_adapter = sum(t[0].numel() for lay in bank.layers for k, t in lay.items() if k not in ("B_gate", "B_up")) + bank.A_dec[0].numel() + bank.B_dec[0].numel()

    def variants(rows):
        return {"a_base": None, "b_lora_all_minus1": [-1] * rows, "c_lora_shared": [0] * rows, "d_lora_distinct": list(range(rows))}

    def run(rows, adapters, steps):
        t0 = time.perf_counter()
        llm.generate_batch(texts[:rows], [pt] * rows, [ps] * rows, forced=forced[:rows], steps_per_poll=64, max_steps=steps, adapters=adapters)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    result = dict(dtype="fp16", rank=args.rank, steps=args.steps, rounds=args.rounds, prefill_rows_per_seq=int(1 + pt.numel() + texts[0].numel() + 1 + ps.numel()),
                  adapter_bytes_per_step=2 * n_adapter, device=torch.cuda.get_device_name(0), decode_step_us={}, prefill_ms={})
    for rows in (8, 32):
        var = variants(rows)
        for ad in var.values():        # warm every shape: workspaces, code objects, the captured graphs
            run(rows, ad, 3)
        step = {k: [] for k in var}
        pre = {k: [] for k in var}
        for _ in range(args.rounds):
            for k, ad in var.items():  # alternate the variants inside a round
                t1 = run(rows, ad, 1)
                tn = run(rows, ad, 1 + args.steps)
                pre[k].append(1e3 * t1)
                step[k].append(1e6 * (tn - t1) / args.steps)
        result["decode_step_us"][str(rows)] = {k: dict(median=round(statistics.median(v), 1), min=round(min(v), 1), max=round(max(v), 1)) for k, v in step.items()}
        if rows == 8:                  # prefill + head + first sample of 8 x 282 rows (one decode step is not subtracted)
            result["prefill_ms"]["8"] = {k: dict(median=round(statistics.median(v), 2), min=round(min(v), 2), max=round(max(v), 2)) for k, v in pre.items()}
        print(rows, "rows", json.dumps(result["decode_step_us"][str(rows)]), flush=True)
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
