"""What a server optimiser step costs.

(a) step: the fused step (ops/csrc/server_opt.hip, one launch) against
    the eager composition of the same rule (fused.server_opt_step_eager,
    the CPU-fallback expression, run on GPU tensors), for the four kinds
    with and without noise at the ResNet-18 and BERT-base parameter
    counts.  Reports microseconds and effective GB/s; both GB/s figures
    use the bytes the FUSED kernel must move (4 bytes x P x streams:
    x, d, m read, x, m written, plus v read and written for the adaptive
    kinds, plus z read with noise), so the eager figure is a rate of
    useful bytes, not of what its dozen passes and temporaries move.
(b) round: the round time of a bench.py preset with the optimiser off
    and with one on.  One engine per configuration in one process, rounds
    alternated so drift hits all of them alike; a second off engine gives
    the off-vs-off spread.

All timings are device-synchronised and follow a warm-up.

Usage (on the GPU box):
    python tools/serveroptbench.py step  [--iters 20] [--sizes resnet18,bert-base]
    python tools/serveroptbench.py round [--preset resnet-10k] [--kind adam]
"""

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from olearning_sim_amd.ops import fused  # noqa: E402

# parameter counts of the two flagship models (ResNet-18 with 100
# classes, BERT-base), as profiles/clip_norm_r09.md lists them
PARAMS = {"resnet18": 11_220_132, "bert-base": 108_625_722}

W, LR, B1, B2, TAU, SIGMA = 1250.0, 0.1, 0.9, 0.99, 1e-3, 1e-4


def step_streams(kind, noise):
    """fp32 streams over P the fused kernel reads plus writes."""
    return (5 if kind == "momentum" else 7) + (1 if noise else 0)


def _time(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(iters + 1)]
    ev[0].record()
    for i in range(iters):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize()
    return [ev[i].elapsed_time(ev[i + 1]) * 1e3 for i in range(iters)]


def cmd_step(args):
    for name in args.sizes.split(","):
        P = PARAMS[name] if name in PARAMS else int(name)
        g = torch.Generator(device="cuda").manual_seed(0)
        x = torch.randn(P, generator=g, device="cuda")
        d = torch.randn(P, generator=g, device="cuda") * W * 1e-3
        z = torch.randn(P, generator=g, device="cuda")
        for kind in fused.SERVER_OPT_KINDS:
            for noise in (False, True):
                row = {"size": name, "params": P, "kind": kind,
                       "noise": noise}
                nbytes = 4 * P * step_streams(kind, noise)
                row["bytes"] = nbytes
                for impl, fn in (("fused", fused.server_opt_step),
                                 ("eager", fused.server_opt_step_eager)):
                    xs = x.clone()
                    m = torch.zeros_like(x)
                    v = (None if kind == "momentum"
                         else torch.full_like(x, TAU * TAU))

                    def run():
                        fn(kind, xs, d, m, v, W, LR, B1, B2, TAU,
                           noise=z if noise else None, sigma=SIGMA)

                    us = _time(run, args.warmup, args.iters)
                    med = statistics.median(us)
                    row[impl + "_us"] = round(med, 2)
                    row[impl + "_us_min"] = round(min(us), 2)
                    row[impl + "_GBs"] = round(nbytes / med / 1e3, 1)
                    del xs, m, v
                row["speedup"] = round(row["eager_us"] / row["fused_us"], 2)
                print(json.dumps(row), flush=True)
        del x, d, z
        torch.cuda.empty_cache()


def _engine(preset_name, clients, **kw):
    import bench  # seeds the MIOpen find-db on import
    from olearning_sim_amd.engine import EngineJob, LogicalEngine
    preset = dict(bench.PRESETS[preset_name])
    preset.pop("force_cpu", None)
    per_gpu = preset.pop("clients_per_gpu")
    job = EngineJob(task_id=f"serveroptbench_{preset_name}",
                    clients=clients or per_gpu, cohort_size=0, rounds=10 ** 6,
                    seed=1234, device="cuda:0", dynamic_num=10 ** 9,
                    **preset, **kw)
    return LogicalEngine(job)


def _timed_round(eng, r):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.run_round(r)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def cmd_round(args):
    engines = {
        "off": _engine(args.preset, args.clients),
        "off_b": _engine(args.preset, args.clients),
        args.kind: _engine(args.preset, args.clients,
                           server_optimizer=args.kind,
                           server_lr=args.server_lr),
    }
    times = {k: [] for k in engines}
    for r in range(args.warmup + args.rounds):
        for name, eng in engines.items():
            ms = _timed_round(eng, r)
            if r >= args.warmup:
                times[name].append(ms)
    med = {k: statistics.median(v) for k, v in times.items()}
    print(json.dumps({
        "preset": args.preset, "rounds": args.rounds, "warmup": args.warmup,
        "kind": args.kind, "server_lr": args.server_lr,
        "ms_median": {k: round(v, 2) for k, v in med.items()},
        "ms_min": {k: round(min(v), 2) for k, v in times.items()},
        "ms_all": {k: [round(x, 2) for x in v] for k, v in times.items()},
        "off_vs_off_pct": round(100 * (med["off_b"] / med["off"] - 1), 3),
        "on_overhead_pct": round(100 * (med[args.kind] / med["off"] - 1), 3),
    }))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    s = sub.add_parser("step")
    s.add_argument("--sizes", default="resnet18,bert-base",
                   help="comma list of names in PARAMS or element counts")
    s.add_argument("--iters", type=int, default=20)
    s.add_argument("--warmup", type=int, default=3)
    s.set_defaults(fn=cmd_step)
    r = sub.add_parser("round")
    r.add_argument("--preset", default="resnet-10k")
    r.add_argument("--clients", type=int, default=0)
    r.add_argument("--rounds", type=int, default=6)
    r.add_argument("--warmup", type=int, default=2)
    r.add_argument("--kind", default="adam",
                   choices=fused.SERVER_OPT_KINDS)
    r.add_argument("--server-lr", type=float, default=0.01)
    r.set_defaults(fn=cmd_round)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "serveroptbench needs a GPU"
    args.fn(args)


if __name__ == "__main__":
    main()
