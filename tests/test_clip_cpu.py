"""Per-client update clipping and server noise on the CPU paths: the
three ops against fp64, the engine's clipped update rule, the noise
mechanism, the control-plane mapping.  The HIP kernels are checked in
test_clip_gpu.py."""

import json
import math
import multiprocessing as mp
import os

import pytest
import torch

import kernel_bounds as kb
from olearning_sim_amd.engine import EngineJob, LogicalEngine
from olearning_sim_amd.ops import fused


def _job(**kw):
    base = dict(task_id="t_clip", model_name="mlp",
                model_kwargs={"in_features": 64, "hidden": 32,
                              "num_classes": 10},
                clients=10, rounds=1, local_steps=2, batch_size=4,
                lr=0.1, device="cpu", dtype="float32", num_classes=10,
                shard_size=16, seed=7)
    base.update(kw)
    return EngineJob(**base)


def _master_after(rounds=1, **kw):
    eng = LogicalEngine(_job(**kw))
    start = eng.master.flat.clone()
    recs = [eng.run_round(r) for r in range(rounds)]
    return start, eng.master.flat.clone(), recs


# ---------------------------------------------------------------------------
# ops

def test_sqnorm_cpu_matches_fp64():
    g = torch.Generator().manual_seed(0)
    C = 5
    shapes = [(7,), (3, 11), (64,)]
    glob = [torch.randn(*s, generator=g) for s in shapes]
    cli = [m.unsqueeze(0) + 1e-3 * torch.randn(C, *s, generator=g)
           for m, s in zip(glob, shapes)]
    sq = fused.client_delta_sqnorm(cli, glob)
    assert sq.shape == (C,) and sq.dtype == torch.float32
    ref = sum(((kb.upcast(c) - kb.upcast(m).unsqueeze(0)) ** 2)
              .reshape(C, -1).sum(1) for c, m in zip(cli, glob))
    n = sum(m.numel() for m in glob)
    kb.assert_bounded(sq, ref, ref, n + 4, torch.float32, label="cpu.sq")


def test_clip_weights_cpu_matches_fp64():
    S = 1.5                                  # S*S = 2.25 exact in fp32
    sq = torch.tensor([0.0, 1.0, 2.25, 2.2500002, 9.0, 1e6, 400.0])
    w = torch.tensor([1.0, 0.5, 1.0, 1.0, 0.25, 1.0, 0.0])
    w_eff, wsum = fused.clip_weights(sq, w, S)
    q = kb.upcast(sq)
    s = torch.where(q > S * S, S / q.sqrt(), torch.ones_like(q))
    ref = kb.upcast(w) * s
    kb.assert_bounded(w_eff, ref, ref.abs(), 1, torch.float32,
                      intrinsic=True, label="cpu.w_eff")
    # not clipped: the weight itself, bit for bit
    assert torch.equal(w_eff[:3], w[:3])
    assert wsum.shape == (1,)
    C = sq.numel()
    assert abs(float(wsum) - float(kb.upcast(w_eff).sum())) \
        <= (C + 2) * 2.0 ** -23 * float(w_eff.abs().sum())


def test_weighted_delta_accum_cpu_takes_tensor_wsum():
    g = torch.Generator().manual_seed(1)
    C, n = 4, 9
    m = torch.randn(n, generator=g)
    buf = m + 0.1 * torch.randn(C, n, generator=g)
    w = torch.rand(C, generator=g)
    d1, d2 = torch.zeros(n), torch.zeros(n)
    fused.weighted_delta_accum([d1], [buf], [m], w, wsum=float(w.sum()))
    fused.weighted_delta_accum([d2], [buf], [m], w, wsum=w.sum().reshape(1))
    assert torch.equal(d1, d2)
    ref, scale, _ = kb.delta_math(torch.zeros(n, dtype=torch.float64),
                                  kb.upcast(buf).reshape(-1), kb.upcast(m),
                                  kb.upcast(w), [0, n], C)
    kb.assert_bounded(d2, ref, scale, C, torch.float32, label="cpu.delta")


# ---------------------------------------------------------------------------
# engine

def test_single_client_update_is_scaled_to_the_clip_norm():
    start, plain, _ = _master_after(clients=1)
    upd = plain - start
    norm = float(upd.double().norm())
    S = norm / 3
    _, clipped, recs = _master_after(clients=1, clip_norm=S)
    # one client of weight 1: master += s * delta with s = S/||delta||
    want = start + upd * (S / norm)
    torch.testing.assert_close(clipped, want, rtol=1e-5, atol=1e-7)
    assert recs[0]["clipped"] == 1
    assert recs[0]["update_norm_mean"] == pytest.approx(norm, rel=1e-5)
    # a bound above the norm leaves the update alone
    _, loose, recs = _master_after(clients=1, clip_norm=2 * norm)
    assert torch.equal(loose, plain)
    assert recs[0]["clipped"] == 0


def test_clipped_master_is_chunk_invariant():
    _, ref, recs = _master_after(update_norm_stats=True)
    S = 0.5 * recs[0]["update_norm_mean"]
    _, m2, r2 = _master_after(clip_norm=S, chunk_clients=2)
    _, m5, r5 = _master_after(clip_norm=S, chunk_clients=5)
    assert torch.allclose(m2, m5, atol=1e-5)
    assert r2[0]["clipped"] == r5[0]["clipped"] > 0
    assert not torch.allclose(m2, ref, atol=1e-5)


def test_stats_only_leaves_the_master_alone():
    _, plain, r0 = _master_after()
    _, stats, r1 = _master_after(update_norm_stats=True)
    assert torch.equal(plain, stats)
    assert "clipped" not in r0[0] and "update_norm_mean" not in r0[0]
    assert r1[0]["clipped"] == 0 and r1[0]["update_norm_mean"] > 0


def test_dropped_clients_are_not_counted():
    def drop_some(round_idx, cohort):
        dropped = torch.zeros(cohort, dtype=torch.bool)
        dropped[:4] = True
        return torch.zeros(cohort, dtype=torch.bool), dropped

    eng = LogicalEngine(_job(clip_norm=1e-6, chunk_clients=4),
                        behavior=drop_some)
    rec = eng.run_round(0)
    # 10 clients in chunks of 4: 4 dropped, 2 tail pads, 6 live
    assert rec["clipped"] == 6


def test_clipped_frac_reaches_the_performance_table():
    from olearning_sim_amd.perf.manager import PerformanceManager
    perf = PerformanceManager()
    eng = LogicalEngine(_job(clip_norm=1e-6, rounds=2), perf=perf)
    eng.run()
    rows = perf.metrics("t_clip", "clipped_frac")
    assert [r["round"] for r in rows] == [0, 1]
    assert all(r["value"] == 1.0 for r in rows)
    quiet = PerformanceManager()
    LogicalEngine(_job(), perf=quiet).run()
    assert quiet.metrics("t_clip", "clipped_frac") == []


def test_noise_is_reproducible_and_differs_between_rounds():
    kw = dict(clip_norm=0.05, noise_multiplier=1.0, rounds=2)
    _, a, _ = _master_after(**kw)
    _, b, _ = _master_after(**kw)
    assert torch.equal(a, b)
    _, clean, _ = _master_after(clip_norm=0.05, rounds=2)
    assert not torch.equal(a, clean)
    # lr = 0: no client update, so each round's master change is its noise
    eng = LogicalEngine(_job(lr=0.0, clip_norm=0.05, noise_multiplier=1.0))
    m0 = eng.master.flat.clone()
    eng.run_round(0)
    m1 = eng.master.flat.clone()
    eng.run_round(1)
    n0, n1 = m1 - m0, eng.master.flat - m1
    assert float(n0.abs().max()) > 0 and not torch.allclose(n0, n1)


def test_resumed_run_draws_the_same_noise(tmp_path):
    kw = dict(clip_norm=0.05, noise_multiplier=1.0, save_every_round=True)
    whole = LogicalEngine(_job(rounds=2, checkpoint_dir=str(tmp_path / "a"),
                               **kw))
    whole.run()
    part = str(tmp_path / "b")
    LogicalEngine(_job(rounds=1, checkpoint_dir=part, **kw)).run()
    resumed = LogicalEngine(_job(rounds=2, checkpoint_dir=part, resume=True,
                                 **kw))
    assert resumed.start_round == 1
    resumed.run()
    assert torch.equal(whole.master.flat, resumed.master.flat)


def test_noise_has_the_stated_standard_deviation():
    S, z = 0.05, 2.0
    _, clean, _ = _master_after(clip_norm=S)
    _, noisy, _ = _master_after(clip_norm=S, noise_multiplier=z)
    noise = (noisy - clean).double()
    P = noise.numel()
    sigma = z * S / 10            # total_weight: 10 clients of weight 1
    # sampling error of a standard deviation over P draws: sigma/sqrt(2P)
    assert abs(float(noise.std()) - sigma) <= 5 / math.sqrt(2 * P) * sigma
    assert abs(float(noise.mean())) <= 5 * sigma / math.sqrt(P)


def test_no_noise_without_weight():
    strategy = json.dumps({"offline_simulation": {"offline_probability": 1.0}})
    eng = LogicalEngine(_job(clip_norm=0.05, noise_multiplier=1.0,
                             behavior_strategy=strategy, dynamic_num=100))
    before = eng.master.flat.clone()
    eng.run_round(0)
    assert torch.equal(before, eng.master.flat)


@pytest.mark.parametrize("kw", [dict(clip_norm=-1.0),
                                dict(clip_norm=1.0, noise_multiplier=-0.5),
                                dict(noise_multiplier=1.0)])
def test_bad_values_raise(kw):
    with pytest.raises(ValueError):
        LogicalEngine(_job(**kw))


def test_operator_params_reach_the_engine_job():
    from test_manager import task_json
    from olearning_sim_amd.task.allocation import HybridOptimizer
    from olearning_sim_amd.task.runner import engine_job_from_task
    from olearning_sim_amd.task.schema import json2taskconfig
    cfg = json2taskconfig(task_json(params={
        "clip_norm": 0.25, "noise_multiplier": 1.1,
        "update_norm_stats": True}))
    job = engine_job_from_task(cfg, HybridOptimizer(cfg).allocate())
    assert job.clip_norm == 0.25 and job.noise_multiplier == 1.1
    assert job.update_norm_stats is True
    cfg = json2taskconfig(task_json())
    job = engine_job_from_task(cfg, HybridOptimizer(cfg).allocate())
    assert job.clip_norm == 0.0 and job.noise_multiplier == 0.0
    assert job.update_norm_stats is False


def test_defaults_never_compute_the_norms(monkeypatch):
    calls = {"sq": 0, "clip": 0}
    real_sq, real_clip = fused.client_delta_sqnorm, fused.clip_weights

    def sq(*a, **k):
        calls["sq"] += 1
        return real_sq(*a, **k)

    def clip(*a, **k):
        calls["clip"] += 1
        return real_clip(*a, **k)

    monkeypatch.setattr(fused, "client_delta_sqnorm", sq)
    monkeypatch.setattr(fused, "clip_weights", clip)
    LogicalEngine(_job(chunk_clients=5)).run_round(0)
    assert calls == {"sq": 0, "clip": 0}
    LogicalEngine(_job(chunk_clients=5, update_norm_stats=True)).run_round(0)
    assert calls == {"sq": 2, "clip": 0}
    LogicalEngine(_job(chunk_clients=5, clip_norm=1.0)).run_round(0)
    assert calls == {"sq": 4, "clip": 2}


# ---------------------------------------------------------------------------
# two ranks over gloo: the noise must not depend on the rank

def _worker(rank, world, port, conn):
    os.environ.update({
        "RANK": str(rank), "WORLD_SIZE": str(world),
        "LOCAL_RANK": str(rank), "MASTER_ADDR": "127.0.0.1",
        "MASTER_PORT": str(port),
    })
    import torch.distributed as dist
    from olearning_sim_amd.parallel import dist as pdist

    ctx = pdist.init_distributed(device="cpu")
    job = EngineJob(task_id="dist_clip", model_name="mlp",
                    model_kwargs={"in_features": 32, "hidden": 16,
                                  "num_classes": 5},
                    clients=4, rounds=2, local_steps=1, batch_size=4,
                    lr=0.1, device="cpu", dtype="float32", num_classes=5,
                    shard_size=8, seed=77, clip_norm=1e-3,
                    noise_multiplier=1.0)
    eng = LogicalEngine(job, dist_ctx=ctx)
    start = eng.master.flat.clone()
    out = eng.run()
    # bytes, not a tensor: see test_dist_gloo.py
    conn.send({"rank": rank,
               "master_bytes": eng.master.flat.numpy().tobytes(),
               "moved": float((eng.master.flat - start).abs().max()),
               "clipped": [r["clipped"] for r in out["records"]]})
    conn.recv()
    dist.destroy_process_group()


def _spawn_round(port):
    ctx = mp.get_context("spawn")
    pipes, procs = [], []
    for rank in range(2):
        parent, child = ctx.Pipe()
        p = ctx.Process(target=_worker, args=(rank, 2, port, child))
        p.start()
        pipes.append(parent)
        procs.append(p)
    results, ok = [], True
    for pipe, p in zip(pipes, procs):
        if pipe.poll(60):
            results.append(pipe.recv())
            pipe.send("ack")
        else:
            ok = False
    for p in procs:
        p.join(30)
        if p.exitcode != 0:
            ok = False
    return ok, results


@pytest.mark.timeout(240)
def test_two_rank_gloo_noise_keeps_masters_equal():
    import socket
    # fresh port per attempt, as in test_dist_gloo.py
    for attempt in range(3):
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        ok, results = _spawn_round(port)
        if ok:
            break
    assert ok, "gloo rendezvous failed 3 times"
    r0, r1 = sorted(results, key=lambda r: r["rank"])
    assert r0["master_bytes"] == r1["master_bytes"]
    # sigma = 1e-3 / 8: the noise, not the clipped update, moved the master
    assert r0["moved"] > 1e-4
    # the counts rode in the stats all-reduce: 4 clients per rank
    assert r0["clipped"] == r1["clipped"] == [8, 8]
