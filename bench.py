#!/usr/bin/env python3
"""Flagship benchmark: FedAvg CNN federated-simulation throughput.

One step = one full FL round: cohort selection -> per-client local
training (client-batched on GPU, E local SGD steps each) -> weighted
delta aggregation (HIP kernel) -> RCCL all-reduce across GPUs -> global
model update.  Weak scaling: each GPU simulates a fixed shard of
clients (default 1250 -> 10k clients at 8 GPUs, BASELINE config 3).

value = whole-job virtual clients trained per second (aggregate over
all ranks); rounds/sec is value / clients_per_round.

Run:  python bench.py --gpus N --steps K --warmup W
A plain run sets up, warms up, times the K steps and prints one JSON
result line; `--dump-outputs DIR` also writes the last timed round's
outputs as DIR/<name>.npy (same arguments -> same inputs, so two builds
compare output for output).  Measurements beyond the headline figure
belong behind `--full`.
For N>1 the driver launches it under torch.distributed.run with one
rank per GPU (RANK/LOCAL_RANK/WORLD_SIZE read from the env).
"""

from __future__ import annotations

import argparse
import json
import os
import shutil
import sys
import tempfile
import time


def _seed_miopen_find_db() -> None:
    """Seed MIOpen's user find-db from the in-repo tuned copy so a fresh
    process skips the ~40 s per-shape Find phase (the db ships the
    gfx950 solver choices for the preset conv shapes; MIOpen wants the
    directory writable, so it is copied to a temp dir)."""
    if os.environ.get("MIOPEN_USER_DB_PATH"):
        return
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                       "olearning_sim_amd", "ops", "miopen_udb")
    if not os.path.isdir(src):
        return
    dst = os.path.join(tempfile.gettempdir(),
                       f"olsim_miopen_udb_{os.getuid()}")
    os.makedirs(dst, exist_ok=True)
    for f in os.listdir(src):
        target = os.path.join(dst, f)
        if not os.path.exists(target):
            # atomic publish: 8 ranks race to seed the same directory
            tmp = target + f".tmp{os.getpid()}"
            shutil.copy2(os.path.join(src, f), tmp)
            os.replace(tmp, target)
    os.environ["MIOPEN_USER_DB_PATH"] = dst


_seed_miopen_find_db()

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from olearning_sim_amd.engine import EngineJob, LogicalEngine  # noqa: E402
from olearning_sim_amd.parallel import dist as pdist  # noqa: E402

PRESETS = {
    # BASELINE config 2: LeNet CIFAR-10, 1k clients, bf16, 1 GPU
    "lenet-1k": dict(model_name="lenet", model_kwargs={"num_classes": 10},
                     clients_per_gpu=1000, num_classes=10, local_steps=2,
                     batch_size=16, lr=0.05, dtype="bfloat16"),
    # BASELINE config 3 (flagship): ResNet-18 CIFAR-100 non-IID, 10k @ 8 GPUs
    "resnet-10k": dict(model_name="resnet18", model_kwargs={"num_classes": 100},
                       clients_per_gpu=1250, num_classes=100, local_steps=2,
                       batch_size=16, lr=0.05, dtype="bfloat16",
                       dirichlet_alpha=0.1),
    # BASELINE config 4: FedProx + deviceflow churn, 50k @ 8 GPUs
    "fedprox-churn-50k": dict(
        model_name="lenet", model_kwargs={"num_classes": 10},
        clients_per_gpu=6250, num_classes=10, local_steps=2, batch_size=16,
        lr=0.05, prox_mu=0.01, dtype="bfloat16",
        behavior_strategy=json.dumps({
            "offline_simulation": {"offline_probability": 0.05,
                                   "spike_period": 5,
                                   "spike_offline_fraction": 0.5},
            "real_time_dispatch": {"use_strategy": True,
                                   "drop_simulation": {"drop_probability": 0.02}},
        })),
    # BASELINE config 5: federated BERT-base next-word, 1k clients
    "bert-base": dict(model_name="bert-base", model_kwargs={},
                      clients_per_gpu=125, num_classes=0, local_steps=1,
                      batch_size=4, lr=0.02, dtype="bfloat16",
                      vocab_size=30522, seq_len=128),
    # BASELINE config 1: CPU plumbing path
    "mlp-cpu": dict(model_name="mlp", model_kwargs={}, clients_per_gpu=10,
                    num_classes=10, local_steps=2, batch_size=8, lr=0.1,
                    dtype="float32", force_cpu=True),
}


# --dump-outputs keeps the global model whole up to this many elements
# (fp32: 48 MB) and writes a fixed seeded sample of a larger one
DUMP_MAX_ELEMS = 12 * 1000 * 1000
DUMP_SAMPLE_SEED = 20240229


def _dump_outputs(out_dir: str, eng, record, rank: int) -> None:
    """Write what the last timed round handed back: the aggregated
    global model (what a caller reads from the engine after the round)
    and the round's client counts, as <name>.npy."""
    import numpy as np
    eng._finish_aggregate()       # multi-rank: fold the in-flight reduce
    if rank != 0 or record is None:
        return
    os.makedirs(out_dir, exist_ok=True)
    flat = eng.master.flat.detach().float()
    n = flat.numel()
    if n > DUMP_MAX_ELEMS:
        gen = torch.Generator().manual_seed(DUMP_SAMPLE_SEED)
        idx = torch.randperm(n, generator=gen)[:DUMP_MAX_ELEMS]
        idx = idx.sort().values
        flat = flat[idx.to(flat.device)]
    np.save(os.path.join(out_dir, "global_params.npy"),
            flat.cpu().numpy().astype(np.float32))
    counts = [record["round"], record["success"], record["failed"],
              record["trained"], int(record["round_failed"])]
    np.save(os.path.join(out_dir, "round_counts.npy"),
            np.asarray(counts, dtype=np.float64))
    if record.get("loss") is not None:
        np.save(os.path.join(out_dir, "round_loss.npy"),
                np.asarray([record["loss"]], dtype=np.float64))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--preset", default="resnet-10k", choices=sorted(PRESETS))
    ap.add_argument("--clients-per-gpu", type=int, default=0)
    ap.add_argument("--chunk", type=int, default=0)
    ap.add_argument("--local-steps", type=int, default=0)
    ap.add_argument("--batch", type=int, default=0)
    ap.add_argument("--trace", default="",
                    help="write a torch.profiler chrome trace of the timed "
                         "steps to this path (off by default; adds overhead)")
    ap.add_argument("--op-table", default="",
                    help="write torch.profiler key_averages (op-level GPU "
                         "time attribution) to this path")
    ap.add_argument("--op-stacks", default="",
                    help="write key_averages grouped by python stack "
                         "(slow; finds which call site owns a kernel)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="after the timed steps, write what the last timed "
                         "round produced (global model, round counts) as "
                         "DIR/<name>.npy")
    ap.add_argument("--full", action="store_true",
                    help="also run the measurements and checks beyond the "
                         "headline figure (none exist yet: a plain run does "
                         "only setup, warmup, the timed steps and the result "
                         "line; anything added later goes behind this flag)")
    args = ap.parse_args()

    preset = dict(PRESETS[args.preset])
    force_cpu = preset.pop("force_cpu", False)
    clients_per_gpu = args.clients_per_gpu or preset.pop("clients_per_gpu")
    preset.pop("clients_per_gpu", None)
    if args.local_steps:
        preset["local_steps"] = args.local_steps
    if args.batch:
        preset["batch_size"] = args.batch

    use_gpu = torch.cuda.is_available() and not force_cpu
    ctx = pdist.init_distributed("cpu" if force_cpu else None)
    world = max(1, ctx.world_size)

    job = EngineJob(
        task_id=f"bench_{args.preset}",
        clients=clients_per_gpu, cohort_size=0, rounds=args.steps,
        chunk_clients=args.chunk, seed=1234,
        device=ctx.device if use_gpu else "cpu",
        dynamic_num=10 ** 9,  # never early-abort on simulated churn
        **preset)
    if not use_gpu:
        job.device = "cpu"
        job.dtype = "float32"
        ctx = pdist.DistContext(rank=ctx.rank, world_size=ctx.world_size,
                                local_rank=ctx.local_rank, device="cpu",
                                backend=ctx.backend)

    eng = LogicalEngine(job, dist_ctx=ctx if ctx.enabled else None)

    def sync():
        if use_gpu:
            torch.cuda.synchronize(eng.device)

    for r in range(args.warmup):
        eng.run_round(r)
    pdist.barrier()
    sync()

    profiler = None
    if (args.trace or args.op_table or args.op_stacks) and ctx.rank == 0:
        from torch.profiler import profile, ProfilerActivity
        acts = [ProfilerActivity.CPU]
        if use_gpu:
            acts.append(ProfilerActivity.CUDA)
        profiler = profile(activities=acts,
                           record_shapes=bool(args.op_table),
                           with_stack=bool(args.op_stacks))
        profiler.__enter__()

    t0 = time.perf_counter()
    record = None
    for r in range(args.warmup, args.warmup + args.steps):
        record = eng.run_round(r)
    pdist.barrier()
    sync()
    elapsed = time.perf_counter() - t0

    if args.dump_outputs:
        _dump_outputs(args.dump_outputs, eng, record, ctx.rank)

    if profiler is not None:
        profiler.__exit__(None, None, None)
        if args.trace:
            profiler.export_chrome_trace(args.trace)
        if args.op_table:
            sort = ("self_cuda_time_total" if use_gpu
                    else "self_cpu_time_total")
            with open(args.op_table, "w") as f:
                f.write(profiler.key_averages().table(
                    sort_by=sort, row_limit=60))
                f.write("\n\n== by input shape ==\n")
                f.write(profiler.key_averages(
                    group_by_input_shape=True).table(
                    sort_by=sort, row_limit=40))
        if args.op_stacks:
            sort = ("self_cuda_time_total" if use_gpu
                    else "self_cpu_time_total")
            with open(args.op_stacks, "w") as f:
                f.write(profiler.key_averages(group_by_stack_n=7).table(
                    sort_by=sort, row_limit=25, max_src_column_width=200))

    # MAX over ranks; also gather per-rank timings so a straggler or a
    # rank that failed to initialise is visible in the output
    per_rank = [round(elapsed, 4)]
    if ctx.enabled:
        import torch.distributed as dist
        dev = eng.device if use_gpu else "cpu"
        all_t = torch.zeros(world, dtype=torch.float64, device=dev)
        all_t[ctx.rank] = elapsed
        dist.all_reduce(all_t)
        per_rank = [round(float(x), 4) for x in all_t.tolist()]
        elapsed = max(per_rank)
        # N ranks really initialised (a silent single-rank fallback must
        # not masquerade as an N-GPU number)
        assert dist.get_world_size() == world, \
            f"world_size {dist.get_world_size()} != requested {world}"
    if args.gpus > 1 and world != args.gpus and ctx.rank == 0:
        print(f"WARNING: --gpus {args.gpus} requested but world={world} "
              f"(launch under torch.distributed.run)", file=sys.stderr)

    clients_per_round = clients_per_gpu * world
    value = clients_per_round * args.steps / elapsed
    ms_per_step = elapsed / args.steps * 1000.0

    if ctx.rank == 0:
        out = {
            "metric": "virtual clients/sec (simulated FL rounds, FedAvg CNN)",
            "value": round(value, 2),
            "unit": "clients/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": job.dtype,
            "data": "synthetic",
            "config": {
                "model": job.model_name,
                "preset": args.preset,
                "clients_total": clients_per_round,
                "clients_per_gpu": clients_per_gpu,
                "local_steps": job.local_steps,
                "local_batch": job.batch_size,
                "num_classes": job.num_classes,
                "dirichlet_alpha": job.dirichlet_alpha,
                "rounds_per_s": round(args.steps / elapsed, 4),
                "parallelism": f"dp{world}",
                "global_batch": clients_per_round * job.batch_size,
                "seq_len": job.seq_len or None,
                "per_rank_s": per_rank,
            },
        }
        print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
