"""Server optimisers (FedAvgM, FedAdagrad, FedAdam, FedYogi) on the CPU
paths: the eager rule against fp64 under the bounds of server_opt_ref.py,
the engine's use of it, the checkpoint sidecar, the control-plane mapping.
The HIP kernel is checked in test_server_opt_gpu.py."""

import json
import math
import multiprocessing as mp
import os

import pytest
import torch

import server_opt_ref as sr
from olearning_sim_amd.engine import EngineJob, LogicalEngine
from olearning_sim_amd.engine.checkpoint import (checkpoint_name,
                                                 latest_round,
                                                 server_opt_name)
from olearning_sim_amd.ops import fused


def _job(**kw):
    base = dict(task_id="t_sopt", model_name="mlp",
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
    for r in range(rounds):
        eng.run_round(r)
    return start, eng.master.flat.clone(), eng


# ---------------------------------------------------------------------------
# the op

@pytest.mark.parametrize("noise", [False, True], ids=["plain", "noise"])
@pytest.mark.parametrize("kind", sr.KINDS)
def test_cpu_step_matches_fp64(kind, noise):
    sc = sr.scalars()
    for n in sr.SIZES:
        x0, d0, m0, v0, z0 = sr.inputs(n)
        x, d, m, v = x0.clone(), d0.clone(), m0.clone(), v0.clone()
        z = z0.clone() if noise else None
        fused.server_opt_step(kind, x, d, m, None if kind == "momentum"
                              else v, sr.W, sr.LR, sr.B1, sr.B2, sr.TAU,
                              noise=z, sigma=sr.SIGMA)
        ref = sr.reference(kind, x0, d0, m0, v0, z, sc)
        sr.assert_step_bounded(kind, x, m, v, ref, v0,
                               f"cpu.{kind}.{int(noise)}.n{n}")
        assert torch.equal(d, d0) and (z is None or torch.equal(z, z0))
        if kind == "momentum":
            assert torch.equal(v, v0)


def _standin(kind, n, mutant):
    """step_math in fp32 (the scalars as Python floats at their fp32
    values), checked like a kernel result."""
    sc = sr.scalars()
    x0, d0, m0, v0, z0 = sr.inputs(n)
    out = sr.step_math(kind, x0, d0, m0, v0, z0, sc, mutant=mutant)
    assert out["x"].dtype == torch.float32
    ref = sr.reference(kind, x0, d0, m0, v0, z0, sc)
    return sr.assert_step_bounded(kind, out["x"], out["m"], out["v"], ref,
                                  v0, f"standin.{kind}.{mutant}")


@pytest.mark.parametrize("kind", sr.KINDS)
def test_bounds_accept_an_fp32_standin(kind):
    worst = _standin(kind, 100003, None)
    assert max(worst.values()) <= 1.0


@pytest.mark.parametrize("kind", ["adagrad", "adam", "yogi"])
def test_bounds_reject_a_dropped_tau(kind):
    with pytest.raises(AssertionError, match=r"\.x: worst element"):
        _standin(kind, 100003, "no_tau")


def test_bounds_reject_a_flipped_yogi_sign():
    with pytest.raises(AssertionError, match=r"\.v: worst element"):
        _standin("yogi", 100003, "flip_sign")


def test_two_adam_steps_by_hand():
    """b1 = 0.5, b2 = 0.75, tau = 0.5 (v0 = 0.25), lr = 1, W = 3.

    Step 1, g = d/3 = [1, -2, 0]:
      m = 0.5*g = [0.5, -1, 0]
      v = 0.75*0.25 + 0.25*g^2 = [0.4375, 1.1875, 0.1875]
      x = [1, -2, 0.5] + m/(sqrt(v) + 0.5)
    Step 2, g = [0, 1, -1]:
      m = 0.5*m + 0.5*g = [0.25, 0, -0.5]
      v = 0.75*v + 0.25*g^2 = [0.328125, 1.140625, 0.390625]
      x += m/(sqrt(v) + 0.5);  sqrt(0.390625) = 0.625"""
    x = torch.tensor([1.0, -2.0, 0.5])
    m = torch.zeros(3)
    v = torch.full((3,), 0.25)
    args = (3.0, 1.0, 0.5, 0.75, 0.5)
    fused.server_opt_step("adam", x, torch.tensor([3.0, -6.0, 0.0]), m, v,
                          *args)
    x1 = [1 + 0.5 / (math.sqrt(0.4375) + 0.5),
          -2 - 1.0 / (math.sqrt(1.1875) + 0.5), 0.5]
    assert x1[0] == pytest.approx(1.4305009, rel=1e-6)
    assert x1[1] == pytest.approx(-2.6290396, rel=1e-6)
    torch.testing.assert_close(m, torch.tensor([0.5, -1.0, 0.0]))
    torch.testing.assert_close(v, torch.tensor([0.4375, 1.1875, 0.1875]))
    torch.testing.assert_close(x, torch.tensor(x1), rtol=1e-6, atol=0)
    fused.server_opt_step("adam", x, torch.tensor([0.0, 3.0, -3.0]), m, v,
                          *args)
    x2 = [x1[0] + 0.25 / (math.sqrt(0.328125) + 0.5), x1[1],
          0.5 - 0.5 / 1.125]
    torch.testing.assert_close(m, torch.tensor([0.25, 0.0, -0.5]))
    torch.testing.assert_close(
        v, torch.tensor([0.328125, 1.140625, 0.390625]))
    torch.testing.assert_close(x, torch.tensor(x2), rtol=1e-6, atol=0)


def test_unknown_kind_raises_in_the_op():
    t = torch.zeros(4)
    with pytest.raises(ValueError):
        fused.server_opt_step("sgd", t, t.clone(), t.clone(), t.clone(),
                              1.0, 1.0, 0.9, 0.99, 1e-3)


# ---------------------------------------------------------------------------
# engine

def test_default_path_is_todays_and_never_calls_the_step(monkeypatch):
    calls = []
    real = fused.server_opt_step
    monkeypatch.setattr(fused, "server_opt_step",
                        lambda *a, **k: calls.append(a) or real(*a, **k))
    start, plain, eng = _master_after()
    assert eng.server_opt is None
    want = start.clone()
    fused.apply_aggregate([want], [eng._delta], 10.0)
    assert torch.equal(plain, want)
    # and with noise: apply_aggregate, then the noise on top
    _, noisy, eng = _master_after(clip_norm=0.05, noise_multiplier=1.0)
    want = start.clone()
    fused.apply_aggregate([want], [eng._delta], 10.0)
    sigma, z = eng._noise(0, 10.0)
    want.add_(z, alpha=sigma)
    assert torch.equal(noisy, want)
    assert calls == []
    _master_after(server_optimizer="adam")
    assert len(calls) == 1


def test_momentum_without_momentum_is_fedavg():
    start, plain, _ = _master_after(rounds=2)
    _, mom, eng = _master_after(rounds=2, server_optimizer="momentum",
                                server_beta1=0.0, server_lr=1.0)
    assert torch.allclose(mom, plain, rtol=1e-6)
    assert eng.server_opt.steps == 2 and eng.server_opt.v is None
    _, full, _ = _master_after(server_optimizer="momentum",
                               server_beta1=0.0)
    _, half, _ = _master_after(server_optimizer="momentum",
                               server_beta1=0.0, server_lr=0.5)
    assert float((full - start).abs().max()) > 1e-4
    assert torch.allclose(half - start, 0.5 * (full - start), rtol=1e-4,
                          atol=1e-7)


@pytest.mark.parametrize("kind", sr.KINDS)
def test_engine_round_follows_the_rule(kind):
    start, got, eng = _master_after(server_optimizer=kind, server_lr=0.1)
    so = eng.server_opt
    P = start.numel()
    v0 = torch.full((P,), 1e-3 * 1e-3)
    ref = sr.reference(kind, start, eng._delta, torch.zeros(P), v0, None,
                       sr.scalars(total_weight=10.0, sigma=0.0, lr=0.1,
                                  b1=0.9, b2=0.99, tau=1e-3))
    sr.assert_step_bounded(kind, got, so.m, so.v, ref, v0,
                           f"engine.cpu.{kind}", shares=False)
    assert so.steps == 1


def test_round_without_weight_takes_no_step():
    strategy = json.dumps({"offline_simulation": {"offline_probability": 1.0}})
    eng = LogicalEngine(_job(server_optimizer="adam", clip_norm=0.05,
                             noise_multiplier=1.0,
                             behavior_strategy=strategy, dynamic_num=100))
    so = eng.server_opt
    before = (eng.master.flat.clone(), so.m.clone(), so.v.clone())
    eng.run_round(0)
    assert torch.equal(before[0], eng.master.flat)
    assert torch.equal(before[1], so.m) and torch.equal(before[2], so.v)
    assert so.steps == 0
    assert float(so.v[0]) == pytest.approx(1e-6) and not so.m.any()


def test_noise_enters_the_pseudo_gradient():
    """Client lr = 0: the delta is exactly zero and g = sigma * z, so one
    round moves the master by server_lr * m / (sqrt(v) + tau) of that g,
    not by that plus sigma * z."""
    S, mult, slr, b1, b2, tau = 0.05, 1.0, 0.5, 0.9, 0.99, 1e-3
    job = _job(lr=0.0, clip_norm=S, noise_multiplier=mult,
               server_optimizer="adam", server_lr=slr)
    eng = LogicalEngine(job)
    start = eng.master.flat.clone()
    eng.run_round(0)
    assert not eng._delta.any()
    gen = torch.Generator().manual_seed(
        (job.seed * 1_000_003 + 0 * 7919 + 0x5EED) % (2 ** 63))
    z = torch.randn(start.shape, generator=gen).double()
    g = (mult * S / 10.0) * z
    m = (1 - b1) * g
    v = b2 * tau * tau + (1 - b2) * g * g
    step = slr * m / (v.sqrt() + tau)
    moved = (eng.master.flat - start).double()
    assert float(step.abs().max()) > 1e-3
    assert torch.allclose(moved, step, rtol=1e-4, atol=1e-7)
    assert not torch.allclose(moved, step + g, rtol=1e-2, atol=1e-5)
    assert not torch.allclose(moved, g, rtol=1e-2, atol=1e-5)


def test_resume_restores_the_optimiser_state(tmp_path):
    kw = dict(server_optimizer="adam", server_lr=0.05,
              save_every_round=True)
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    whole = LogicalEngine(_job(rounds=3, checkpoint_dir=a, **kw))
    whole.run()
    for r in range(3):
        art = os.path.join(a, checkpoint_name("t_sopt", r))
        assert os.path.exists(art)
        assert os.path.exists(art + ".server_opt.safetensors")
        assert art + ".server_opt.safetensors" == os.path.join(
            a, server_opt_name("t_sopt", r))
    assert latest_round(a, "t_sopt") == 2

    LogicalEngine(_job(rounds=1, checkpoint_dir=b, **kw)).run()
    assert latest_round(b, "t_sopt") == 0
    resumed = LogicalEngine(_job(rounds=3, checkpoint_dir=b, resume=True,
                                 **kw))
    assert resumed.start_round == 1 and resumed.server_opt.steps == 1
    resumed.run()
    assert torch.equal(whole.master.flat, resumed.master.flat)
    assert torch.equal(whole.server_opt.m, resumed.server_opt.m)
    assert torch.equal(whole.server_opt.v, resumed.server_opt.v)
    assert resumed.server_opt.steps == 3
    assert latest_round(b, "t_sopt") == 2

    # the model artifact holds the model alone
    from safetensors.torch import load_file
    names = set(load_file(os.path.join(b, checkpoint_name("t_sopt", 2))))
    assert names == set(whole.master.state_dict())
    side = load_file(os.path.join(b, server_opt_name("t_sopt", 2)))
    assert set(side) == {"m", "v", "step"} and int(side["step"]) == 3

    # the optimiser off needs no sidecar; on, a missing one is an error
    missing = os.path.join(b, server_opt_name("t_sopt", 2))
    os.remove(missing)
    LogicalEngine(_job(rounds=4, checkpoint_dir=b, resume=True,
                       save_every_round=True))
    with pytest.raises(RuntimeError) as err:
        LogicalEngine(_job(rounds=4, checkpoint_dir=b, resume=True, **kw))
    assert missing in str(err.value)


@pytest.mark.parametrize("kw", [
    dict(server_optimizer="sgd"),
    dict(server_optimizer="adam", server_lr=0.0),
    dict(server_optimizer="momentum", server_lr=-1.0),
    dict(server_optimizer="momentum", server_beta1=1.0),
    dict(server_optimizer="adam", server_beta1=-0.1),
    dict(server_optimizer="yogi", server_beta2=1.0),
    dict(server_optimizer="adagrad", server_tau=0.0),
    dict(server_optimizer="adam", server_tau=-1e-3),
    dict(server_optimizer="yogi", server_tau=0.0)])
def test_bad_values_raise(kw):
    with pytest.raises(ValueError):
        LogicalEngine(_job(**kw))


def test_momentum_needs_no_tau():
    LogicalEngine(_job(server_optimizer="momentum", server_tau=0.0))


def test_operator_params_reach_the_engine_job():
    from test_manager import task_json
    from olearning_sim_amd.task.allocation import HybridOptimizer
    from olearning_sim_amd.task.runner import engine_job_from_task
    from olearning_sim_amd.task.schema import json2taskconfig
    cfg = json2taskconfig(task_json(params={
        "server_optimizer": "yogi", "server_lr": 0.3, "server_beta1": 0.8,
        "server_beta2": 0.95, "server_tau": 0.01}))
    job = engine_job_from_task(cfg, HybridOptimizer(cfg).allocate())
    assert job.server_optimizer == "yogi" and job.server_lr == 0.3
    assert (job.server_beta1, job.server_beta2, job.server_tau) \
        == (0.8, 0.95, 0.01)
    cfg = json2taskconfig(task_json())
    job = engine_job_from_task(cfg, HybridOptimizer(cfg).allocate())
    assert job.server_optimizer == ""
    assert (job.server_lr, job.server_beta1, job.server_beta2,
            job.server_tau) == (1.0, 0.9, 0.99, 1e-3)
    assert LogicalEngine(_job()).server_opt is None


# ---------------------------------------------------------------------------
# two ranks over gloo: every rank takes the same step from the same state

def _worker(rank, world, port, conn):
    os.environ.update({
        "RANK": str(rank), "WORLD_SIZE": str(world),
        "LOCAL_RANK": str(rank), "MASTER_ADDR": "127.0.0.1",
        "MASTER_PORT": str(port),
    })
    import torch.distributed as dist
    from olearning_sim_amd.parallel import dist as pdist

    ctx = pdist.init_distributed(device="cpu")
    job = EngineJob(task_id="dist_sopt", model_name="mlp",
                    model_kwargs={"in_features": 32, "hidden": 16,
                                  "num_classes": 5},
                    clients=4, rounds=2, local_steps=1, batch_size=4,
                    lr=0.1, device="cpu", dtype="float32", num_classes=5,
                    shard_size=8, seed=77, clip_norm=1e-3,
                    noise_multiplier=1.0, server_optimizer="yogi",
                    server_lr=0.01)
    eng = LogicalEngine(job, dist_ctx=ctx)
    start = eng.master.flat.clone()
    eng.run()
    # bytes, not a tensor: see test_dist_gloo.py
    conn.send({"rank": rank,
               "master_bytes": eng.master.flat.numpy().tobytes(),
               "m_bytes": eng.server_opt.m.numpy().tobytes(),
               "v_bytes": eng.server_opt.v.numpy().tobytes(),
               "steps": eng.server_opt.steps,
               "moved": float((eng.master.flat - start).abs().max())})
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
def test_two_rank_gloo_yogi_keeps_ranks_equal():
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
    for key in ("master_bytes", "m_bytes", "v_bytes"):
        assert r0[key] == r1[key], key
    assert r0["steps"] == r1["steps"] == 2
    # two Yogi steps of server_lr * m / (sqrt(v) + tau), |m| / sqrt(v)
    # of order 0.1 to 1 after a step from v0 = tau^2
    assert r0["moved"] > 1e-4
