"""What uplink compression costs.

(a) accum: the quantised accumulate over a model's parameter list at a
    given client count, against the plain weighted_delta_accum and against
    client_delta_sqnorm + weighted_delta_accum on the same tensors.  The
    second pairing is what a two-pass design (a scale pass, then the
    accumulate) would read; the single pass has to beat it.  Achieved
    bytes/s from the shapes ((C*P + P) elements x itemsize: every replica
    and the master once), the variants alternated within each iteration.
    The replicas are perturbed first: a replica equal to the master has
    a == 0 in every bucket and the kernel would skip its arithmetic.
(b) round: the round time of a bench.py preset with compression off and
    with each bit width.  One engine per configuration in one process,
    rounds alternated so drift hits all of them alike; a second off engine
    gives the off-vs-off spread.

All timings are device-synchronised and follow a warm-up.

Usage (on the GPU box):
    python tools/quantbench.py accum [--model resnet18 --clients 1250]
    python tools/quantbench.py round [--preset resnet-10k] [--rounds 6]
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


def cmd_accum(args):
    dtype = torch.bfloat16
    model = build_model(args.model, **json.loads(args.model_kwargs))
    gp = model.init_global(device="cpu", dtype=torch.float32,
                           generator=torch.Generator().manual_seed(1234))
    master = FlatParams({k: v.cuda() for k, v in gp.items()})
    cast = master.views_of(master.flat.to(dtype))
    C = args.clients
    params = replicate_params(cast, C)
    plist = [p.detach() for p in params.values()]
    glist = [cast[k] for k in params]
    gen = torch.Generator(device="cuda").manual_seed(1)
    for p in plist:
        # the engine's regime: replicas within lr * grad of the master
        rows = max(1, (1 << 26) // max(1, p[0].numel()))
        for lo in range(0, C, rows):
            blk = p[lo:lo + rows]
            blk.add_((1e-2 * torch.randn(blk.shape, generator=gen,
                                         device="cuda")).to(dtype))
    offs, off = [], 0
    for n in master.numels.values():
        offs.append(off)
        off += n
    P = master.numel()
    nbytes = (C * P + P) * plist[0].element_size()
    w = torch.rand(C, device="cuda") + 0.5
    wsum = float(w.sum())
    ids = torch.arange(C, device="cuda", dtype=torch.int64)
    delta = master.zeros_like_flat()
    dviews = list(master.views_of(delta).values())
    key = fused.uplink_key(1234, 0, 0)

    def plain():
        fused.weighted_delta_accum(dviews, plist, glist, w, wsum=wsum)

    def two_pass():
        fused.client_delta_sqnorm(plist, glist)
        fused.weighted_delta_accum(dviews, plist, glist, w, wsum=wsum)

    def quant(bits):
        return lambda: fused.weighted_delta_accum_quant(
            dviews, plist, glist, w, ids, bits, key, offs)

    variants = {"plain": plain, "sqnorm_plus_plain": two_pass}
    for b in args.bits:
        variants[f"quant{b}"] = quant(b)
    for _ in range(args.warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(args.iters):
        for name, fn in variants.items():
            a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms[name].append(a.elapsed_time(b))
    med = {k: statistics.median(v) for k, v in ms.items()}

    # per parameter, for the list of what holds the quantised pass back
    ops = fused.load_hip_ops(required=True)
    bits = args.bits[-1]
    rows = []
    for name, p, g, d, o in zip(params, plist, glist, dviews, offs):
        fp, fg, fd = p.reshape(-1), g.reshape(-1), d.reshape(-1)
        call = lambda: ops.delta_accum_quant(  # noqa: E731
            fd, fp, fg, w, ids, C, bits, key & 0xFFFFFFFF, key >> 32, o, True)
        for _ in range(2):
            call()
        a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        a.record()
        for _ in range(args.param_iters):
            call()
        b.record()
        torch.cuda.synchronize()
        us = a.elapsed_time(b) * 1e3 / args.param_iters
        n = g.numel()
        rows.append({"name": name, "n": n,
                     "route": ops.delta_accum_quant_route(
                         n, C, 1, fg.data_ptr() % 16 == 0,
                         fp.data_ptr() % 16 == 0),
                     "us": round(us, 2),
                     "TBs": round((C * n + n) * 2 / us / 1e6, 3)})
    rows.sort(key=lambda r: -r["us"])
    print(json.dumps({
        "model": args.model, "clients": C, "params": P,
        "tensors": len(plist), "bytes": nbytes, "iters": args.iters,
        "ms_median": {k: round(v, 4) for k, v in med.items()},
        "ms_min": {k: round(min(v), 4) for k, v in ms.items()},
        "ms_max": {k: round(max(v), 4) for k, v in ms.items()},
        "TBs": {k: round(nbytes / v / 1e9, 3) for k, v in med.items()},
        "of_copy": {k: round(nbytes / v / 1e9 / COPY_TBS, 3)
                    for k, v in med.items()},
        "vs_plain": {k: round(v / med["plain"], 3) for k, v in med.items()},
        "vs_two_pass": {k: round(v / med["sqnorm_plus_plain"], 3)
                        for k, v in med.items()},
        "scalar_route_tensors": sum(r["route"] == "scalar" for r in rows),
        "per_param_bits": bits,
        "sum_param_us": round(sum(r["us"] for r in rows), 1),
        "slowest": rows[:args.top],
    }))


def _engine(preset_name, clients, **kw):
    preset = dict(bench.PRESETS[preset_name])
    preset.pop("force_cpu", None)
    per_gpu = preset.pop("clients_per_gpu")
    job = EngineJob(task_id=f"quantbench_{preset_name}",
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
    engines = {"off": _engine(args.preset, args.clients),
               "off_b": _engine(args.preset, args.clients)}
    for b in args.bits:
        engines[f"bits{b}"] = _engine(args.preset, args.clients,
                                      uplink_bits=b)
    times = {k: [] for k in engines}
    last = {}
    for r in range(args.warmup + args.rounds):
        for name, eng in engines.items():
            ms, rec = _timed_round(eng, r)
            if r >= args.warmup:
                times[name].append(ms)
                last[name] = rec
    med = {k: statistics.median(v) for k, v in times.items()}
    print(json.dumps({
        "preset": args.preset, "rounds": args.rounds, "warmup": args.warmup,
        "ms_median": {k: round(v, 2) for k, v in med.items()},
        "ms_min": {k: round(min(v), 2) for k, v in times.items()},
        "ms_all": {k: [round(x, 2) for x in v] for k, v in times.items()},
        "off_vs_off_pct": round(100 * (med["off_b"] / med["off"] - 1), 3),
        "overhead_pct": {k: round(100 * (v / med["off"] - 1), 3)
                         for k, v in med.items() if k.startswith("bits")},
        "overhead_ms": {k: round(v - med["off"], 2)
                        for k, v in med.items() if k.startswith("bits")},
        "uplink_ratio": {k: last[k]["uplink_ratio"] for k in last
                         if k.startswith("bits")},
        "uplink_bytes_per_client": {k: last[k]["uplink_bytes_per_client"]
                                    for k in last if k.startswith("bits")},
    }))


def _bits(text):
    bits = [int(b) for b in text.split(",")]
    assert all(b in fused.UPLINK_BITS for b in bits), bits
    return bits


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    a = sub.add_parser("accum")
    a.add_argument("--model", default="resnet18")
    a.add_argument("--model-kwargs", default='{"num_classes": 100}')
    a.add_argument("--clients", type=int, default=1250)
    a.add_argument("--bits", type=_bits, default=[2, 4, 8])
    a.add_argument("--iters", type=int, default=10)
    a.add_argument("--warmup", type=int, default=3)
    a.add_argument("--param-iters", type=int, default=5)
    a.add_argument("--top", type=int, default=8)
    a.set_defaults(fn=cmd_accum)
    r = sub.add_parser("round")
    r.add_argument("--preset", default="resnet-10k",
                   choices=sorted(bench.PRESETS))
    r.add_argument("--clients", type=int, default=0)
    r.add_argument("--bits", type=_bits, default=[8])
    r.add_argument("--rounds", type=int, default=6)
    r.add_argument("--warmup", type=int, default=2)
    r.set_defaults(fn=cmd_round)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "quantbench needs a GPU"
    args.fn(args)


if __name__ == "__main__":
    main()
