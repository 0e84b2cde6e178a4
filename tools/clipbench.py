"""What per-client update clipping costs.

(a) round: the round time of a bench.py preset with clipping off, with
    update_norm_stats only, and with clipping plus noise.  One engine per
    configuration in one process, rounds alternated so drift hits all of
    them alike; a second clipping-off engine gives the off-vs-off spread.
(b) sqnorm: the squared-norm pass alone over a model's parameter list at
    a given client count, as achieved bytes/s from the shapes
    ((C*P + P) elements x itemsize), with the slowest parameters listed.

All timings are device-synchronised and follow a warm-up.

Usage (on the GPU box):
    python tools/clipbench.py round  [--preset resnet-10k] [--rounds 6]
    python tools/clipbench.py sqnorm [--model resnet18 --clients 1250]
"""

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import bench  # noqa: E402  (seeds the MIOpen find-db on import)
import torch  # noqa: E402

from olearning_sim_amd.engine import EngineJob, LogicalEngine  # noqa: E402
from olearning_sim_amd.engine.client_manager import (  # noqa: E402
    FlatParams, replicate_params)
from olearning_sim_amd.models import build_model  # noqa: E402
from olearning_sim_amd.ops import fused  # noqa: E402

# streaming float4 copy measured on MI355X (HBM3E, 8.0 TB/s spec)
COPY_TBS = 6.29


def _engine(preset_name, clients, **kw):
    preset = dict(bench.PRESETS[preset_name])
    preset.pop("force_cpu", None)
    per_gpu = preset.pop("clients_per_gpu")
    job = EngineJob(task_id=f"clipbench_{preset_name}",
                    clients=clients or per_gpu, cohort_size=0, rounds=10 ** 6,
                    seed=1234, device="cuda:0", dynamic_num=10 ** 9,
                    **preset, **kw)
    return LogicalEngine(job)


def _timed_round(eng, r):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rec = eng.run_round(r)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, rec


def cmd_round(args):
    # stats-only probe rounds tell which clip norm is in reach of the
    # updates: the norms shrink over the first rounds, so take half the
    # mean of the last probe round
    probe = _engine(args.preset, args.clients, update_norm_stats=True)
    for r in range(args.warmup + 1):
        _, rec = _timed_round(probe, r)
    clip = args.clip_norm or 0.5 * rec["update_norm_mean"]
    del probe
    torch.cuda.empty_cache()
    engines = {
        "off": _engine(args.preset, args.clients),
        "off_b": _engine(args.preset, args.clients),
        "stats": _engine(args.preset, args.clients, update_norm_stats=True),
        "clip_noise": _engine(args.preset, args.clients, clip_norm=clip,
                              noise_multiplier=args.noise),
    }
    times = {k: [] for k in engines}
    last = {}
    for r in range(args.warmup + args.rounds):
        for name, eng in engines.items():
            ms, rec = _timed_round(eng, r)
            if r >= args.warmup:
                times[name].append(ms)
                last[name] = rec
    med = {k: statistics.median(v) for k, v in times.items()}
    out = {
        "preset": args.preset, "rounds": args.rounds, "warmup": args.warmup,
        "clip_norm": clip, "noise_multiplier": args.noise,
        "ms_median": {k: round(v, 2) for k, v in med.items()},
        "ms_min": {k: round(min(v), 2) for k, v in times.items()},
        "ms_all": {k: [round(x, 2) for x in v] for k, v in times.items()},
        "off_vs_off_pct": round(100 * (med["off_b"] / med["off"] - 1), 3),
        "stats_overhead_pct": round(100 * (med["stats"] / med["off"] - 1), 3),
        "clip_noise_overhead_pct": round(
            100 * (med["clip_noise"] / med["off"] - 1), 3),
        "clipped": last["clip_noise"].get("clipped"),
        "update_norm_mean": last["stats"].get("update_norm_mean"),
    }
    print(json.dumps(out))


def cmd_sqnorm(args):
    dtype = torch.bfloat16
    kwargs = json.loads(args.model_kwargs)
    model = build_model(args.model, **kwargs)
    gp = model.init_global(device="cpu", dtype=torch.float32,
                           generator=torch.Generator().manual_seed(1234))
    master = FlatParams({k: v.cuda() for k, v in gp.items()})
    cast = master.views_of(master.flat.to(dtype))
    C = args.clients
    params = replicate_params(cast, C)
    plist = [p.detach() for p in params.values()]
    glist = [cast[k] for k in params]
    P = master.numel()
    nbytes = (C * P + P) * plist[0].element_size()

    def run():
        return fused.client_delta_sqnorm(plist, glist)

    for _ in range(args.warmup):
        run()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(args.iters + 1)]
    ev[0].record()
    for i in range(args.iters):
        run()
        ev[i + 1].record()
    torch.cuda.synchronize()
    ms = [ev[i].elapsed_time(ev[i + 1]) for i in range(args.iters)]
    med = statistics.median(ms)

    # per parameter, for the list of what holds the pass back
    ops = fused.load_hip_ops(required=True)
    sq = torch.zeros(C, device="cuda")
    rows = []
    for name, p, g in zip(params, plist, glist):
        flat_p, flat_g = p.reshape(-1), g.reshape(-1)
        for _ in range(2):
            ops.client_delta_sqnorm(sq, flat_p, flat_g, C)
        a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        a.record()
        for _ in range(args.param_iters):
            ops.client_delta_sqnorm(sq, flat_p, flat_g, C)
        b.record()
        torch.cuda.synchronize()
        us = a.elapsed_time(b) * 1e3 / args.param_iters
        n = g.numel()
        vec = (n % 8 == 0 and flat_p.data_ptr() % 16 == 0
               and flat_g.data_ptr() % 16 == 0)
        rows.append({"name": name, "n": n, "vector": vec,
                     "us": round(us, 2),
                     "TBs": round((C * n + n) * 2 / us / 1e6, 3)})
    rows.sort(key=lambda r: -r["us"])
    tbs = nbytes / med / 1e9
    print(json.dumps({
        "model": args.model, "clients": C, "params": P,
        "tensors": len(plist), "bytes": nbytes,
        "ms_median": round(med, 4), "ms_min": round(min(ms), 4),
        "TBs": round(tbs, 3), "of_copy": round(tbs / COPY_TBS, 3),
        "scalar_path_tensors": sum(not r["vector"] for r in rows),
        "sum_param_us": round(sum(r["us"] for r in rows), 1),
        "slowest": rows[:args.top],
        "below_1TBs_us": round(sum(r["us"] for r in rows
                                   if r["TBs"] < 1.0), 1),
        "below_1TBs_tensors": sum(r["TBs"] < 1.0 for r in rows),
    }))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("round")
    r.add_argument("--preset", default="resnet-10k",
                   choices=sorted(bench.PRESETS))
    r.add_argument("--clients", type=int, default=0)
    r.add_argument("--rounds", type=int, default=6)
    r.add_argument("--warmup", type=int, default=2)
    r.add_argument("--clip-norm", type=float, default=0.0,
                   help="0: the mean update norm of a probe round")
    r.add_argument("--noise", type=float, default=1.0)
    r.set_defaults(fn=cmd_round)
    s = sub.add_parser("sqnorm")
    s.add_argument("--model", default="resnet18")
    s.add_argument("--model-kwargs", default='{"num_classes": 100}')
    s.add_argument("--clients", type=int, default=1250)
    s.add_argument("--iters", type=int, default=10)
    s.add_argument("--warmup", type=int, default=3)
    s.add_argument("--param-iters", type=int, default=5)
    s.add_argument("--top", type=int, default=8)
    s.set_defaults(fn=cmd_sqnorm)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "clipbench needs a GPU"
    args.fn(args)


if __name__ == "__main__":
    main()
