"""Whole federated rounds of bert-base at a long sequence, the fused long
attention (ops/csrc/attn_long.hip) against the library route, in one process.

The job is the benchmark's bert-base preset (125 clients, 1 local step,
lr 0.02, bf16, vocab 30522) with seq_len and batch_size from the arguments;
the default, 256 tokens x batch 2, keeps the preset's 512 tokens per client.
One engine runs every round; OLSIM_ATTN_LONG, read at call time, picks the
route.  After warm-up rounds on both routes the two alternate, --runs
windows of --steps rounds each, a host clock around work that ends in a
device synchronise.  Prints one JSON line: seconds per round per route as
the median over the runs with their min..max spread.

    python tools/attnround.py [--seq-len 256] [--batch 2] [--steps 3]
"""

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from olearning_sim_amd.engine import EngineJob, LogicalEngine   # noqa: E402
from olearning_sim_amd.ops import attn                          # noqa: E402

ROUTES = ("fused", "torch")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seq-len", type=int, default=256)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--clients", type=int, default=125)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "attnround.py needs a GPU"

    total = 2 * (args.warmup + args.runs * args.steps)
    job = EngineJob(task_id="attnround", model_name="bert-base",
                    model_kwargs={"seq_len": args.seq_len},
                    clients=args.clients, cohort_size=0,
                    rounds=total, chunk_clients=0, seed=1234, device="cuda:0",
                    dynamic_num=10 ** 9, num_classes=0, local_steps=1,
                    batch_size=args.batch, lr=0.02, dtype="bfloat16",
                    vocab_size=30522, seq_len=args.seq_len)
    eng = LogicalEngine(job)
    rnd = 0

    def rounds(route, n):
        nonlocal rnd
        os.environ["OLSIM_ATTN_LONG"] = route
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            eng.run_round(rnd)
            rnd += 1
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n

    calls = {}
    for route in ROUTES:
        before = attn.ATTN_LONG_CALLS
        rounds(route, args.warmup)
        calls[route] = attn.ATTN_LONG_CALLS - before
    res = {route: [] for route in ROUTES}
    for _ in range(args.runs):
        for route in ROUTES:
            res[route].append(rounds(route, args.steps))
    out = {"model": "bert-base", "clients": args.clients,
           "batch": args.batch, "seq_len": args.seq_len,
           "steps": args.steps, "runs": args.runs}
    for route, s in res.items():
        out[route + "_s_per_round"] = round(statistics.median(s), 4)
        out[route + "_spread_s"] = [round(min(s), 4), round(max(s), 4)]
        out[route + "_long_calls_in_warmup"] = calls[route]
    out["speedup"] = round(out["torch_s_per_round"]
                           / out["fused_s_per_round"], 3)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
