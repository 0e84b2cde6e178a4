"""The server optimiser kernel (ops/csrc/server_opt.hip) and the engine
that steps with it on the GPU.  Every result is compared with fp64
computed from upcast copies of the tensors the kernel received, under the
bounds derived in server_opt_ref.py."""

import pytest
import torch

import kernel_bounds as kb
import server_opt_ref as sr

pytestmark = pytest.mark.gpu

SENTINEL = 12345.678


@pytest.fixture(scope="module")
def ops():
    from olearning_sim_amd.ops import load_hip_ops
    return load_hip_ops(required=True)


def _place(t, pad):
    """t on the GPU: a fresh tensor (pad 0), or a view pad elements into a
    larger one filled with SENTINEL.  Returns (operand, whole)."""
    if pad == 0:
        dev = t.cuda()
        return dev, dev
    whole = torch.full((t.numel() + 2 * pad,), SENTINEL, device="cuda")
    view = whole[pad:pad + t.numel()]
    view.copy_(t)
    return view, whole


def _aligned(tensors):
    return all(t.data_ptr() % 16 == 0 for t in tensors)


def _step(kind, noise, n, pad=0, empty_v=False, seed=0, **scal):
    """One fused step on GPU copies of inputs(n).  Returns the operands
    after it, their whole tensors, the CPU inputs and the route the
    launcher took for them."""
    from olearning_sim_amd.ops import fused
    cpu = dict(zip("xdmvz", sr.inputs(n, seed)))
    if not noise:
        cpu["z"] = None
    dev, whole = {}, {}
    for k, t in cpu.items():
        if t is not None:
            dev[k], whole[k] = _place(t, pad)
    v_arg = dev["v"]
    if empty_v:
        v_arg = torch.empty(0, device="cuda")
    used = [dev[k] for k in "xdm"] + ([dev["z"]] if noise else [])
    if kind != "momentum":
        used.append(dev["v"])
    route = fused.load_hip_ops(required=True).server_opt_route(
        n, _aligned(used))
    p = dict(total_weight=sr.W, lr=sr.LR, beta1=sr.B1, beta2=sr.B2,
             tau=sr.TAU)
    p.update(scal)
    fused.server_opt_step(kind, dev["x"], dev["d"], dev["m"], v_arg,
                          p["total_weight"], p["lr"], p["beta1"], p["beta2"],
                          p["tau"], noise=dev.get("z"), sigma=sr.SIGMA)
    torch.cuda.synchronize()
    return dev, whole, cpu, route


def _check(kind, dev, cpu, label, **scal):
    sc = sr.scalars(**scal)
    ref = sr.reference(kind, cpu["x"], cpu["d"], cpu["m"], cpu["v"],
                       cpu["z"], sc)
    worst = sr.assert_step_bounded(kind, dev["x"], dev["m"], dev["v"], ref,
                                   cpu["v"], label)
    # d and z are only read; momentum has no v
    assert torch.equal(dev["d"].cpu(), cpu["d"]), label
    if cpu["z"] is not None:
        assert torch.equal(dev["z"].cpu(), cpu["z"]), label
    if kind == "momentum":
        assert torch.equal(dev["v"].cpu(), cpu["v"]), label
    return worst


@pytest.mark.parametrize("noise", [False, True], ids=["plain", "noise"])
@pytest.mark.parametrize("kind", sr.KINDS)
def test_step_bounded(kind, noise):
    for n in sr.SIZES:
        dev, _, cpu, route = _step(kind, noise, n)
        assert route == ("v4" if n >= 4 else "scalar")
        _check(kind, dev, cpu, f"sopt.{kind}.{int(noise)}.n{n}")


def test_momentum_accepts_an_empty_v():
    for n in (3, 100003):
        dev, _, cpu, _ = _step("momentum", True, n, empty_v=True)
        _check("momentum", dev, cpu, f"sopt.momentum.empty_v.n{n}")


@pytest.mark.parametrize("kind", sr.KINDS)
def test_route_follows_alignment_and_both_stay_bounded(ops, kind):
    assert ops.server_opt_route(4, True) == "v4"
    assert ops.server_opt_route(3, True) == "scalar"
    assert ops.server_opt_route(100008, False) == "scalar"
    for n in (3, 1028, 100003):
        dev, _, cpu, route = _step(kind, True, n, pad=0)
        assert route == ("v4" if n >= 4 else "scalar"), n
        _check(kind, dev, cpu, f"route.fresh.{kind}.n{n}")
        # the same data one element into larger tensors
        dev, _, cpu, route = _step(kind, True, n, pad=1)
        assert dev["x"].data_ptr() % 16 == 4 and route == "scalar", n
        _check(kind, dev, cpu, f"route.view.{kind}.n{n}")


@pytest.mark.parametrize("pad,want", [(8, "v4"), (9, "scalar")])
@pytest.mark.parametrize("kind", ["momentum", "yogi"])
def test_no_write_outside_the_operands(kind, pad, want):
    for n in (100003, 5):
        dev, whole, cpu, route = _step(kind, True, n, pad=pad)
        assert route == want
        _check(kind, dev, cpu, f"overrun.{kind}.{want}.n{n}")
        sent = torch.full((pad,), SENTINEL, device="cuda")
        for k, w in whole.items():
            assert w.numel() == n + 2 * pad
            assert torch.equal(w[:pad], sent), (k, "head")
            assert torch.equal(w[pad + n:], sent), (k, "tail")


@pytest.mark.parametrize("kind", sr.KINDS)
def test_two_calls_are_bit_equal(kind):
    a, _, _, _ = _step(kind, True, 100003)
    b, _, _, _ = _step(kind, True, 100003)
    for k in "xmv":
        assert torch.equal(a[k], b[k]), k


def test_momentum_with_beta1_zero_is_plain_fedavg():
    for n in (7, 100003):
        dev, _, cpu, _ = _step("momentum", False, n, lr=1.0, beta1=0.0)
        x0, d = kb.upcast(cpu["x"]), kb.upcast(cpu["d"])
        ref = x0 + d / sr.W
        err = (kb.upcast(dev["x"]) - ref).abs()
        limit = 2 * 2.0 ** -22 * (x0.abs() + d.abs() / sr.W)
        print(f"fedavg n={n}: worst err/limit "
              f"{float((err / limit).max()):.4f}")
        assert bool((err <= limit).all())
        _check("momentum", dev, cpu, f"sopt.fedavg.n{n}", lr=1.0, b1=0.0)


def test_binding_rejects_bad_operands(ops):
    n = 8
    t = [torch.zeros(n, device="cuda") for _ in range(4)]
    tail = (1.0, 0.0, 1.0, 0.9, 0.99, 1e-3)
    ops.server_opt_step(2, *t, None, *tail)
    bad = [
        (2, t[0], t[1][:4], t[2], t[3], None) + tail,         # numel
        (2, t[0], t[1], t[2], t[3][:4], None) + tail,
        (2, t[0], t[1], t[2], t[3], t[0][:4]) + tail,
        (2, t[0], t[1].double(), t[2], t[3], None) + tail,    # dtype
        (2, t[0], t[1], t[2].bfloat16(), t[3], None) + tail,
        (2, t[0], t[1].cpu(), t[2], t[3], None) + tail,       # device
        (2, t[0], t[1], t[2], t[3], t[0].cpu()) + tail,
        (2, t[0], t[1], t[2], t[3], None, 0.0) + tail[1:],    # W = 0
        (2, t[0], t[1], t[2], torch.empty(0, device="cuda"), None) + tail,
        (4, t[0], t[1], t[2], t[3], None) + tail,             # kind
        (2, torch.zeros(2, n, device="cuda").t(), t[1].repeat(2), t[2]
         .repeat(2), t[3].repeat(2), None) + tail,            # contiguous
    ]
    for args in bad:
        with pytest.raises(RuntimeError, match="server_opt_step"):
            ops.server_opt_step(*args)
    torch.cuda.synchronize()
    assert not any(bool(x.any()) for x in t[:3])


# ---------------------------------------------------------------------------
# engine: the bf16 MLP of test_clip_gpu.py's engine tests

def _engine(**kw):
    from olearning_sim_amd.engine import EngineJob, LogicalEngine
    base = dict(task_id="t_sopt_gpu", model_name="mlp",
                model_kwargs={"in_features": 64, "hidden": 32,
                              "num_classes": 10},
                clients=8, rounds=2, local_steps=2, batch_size=8, lr=0.1,
                device="cuda:0", dtype="bfloat16", num_classes=10, seed=5)
    base.update(kw)
    return LogicalEngine(EngineJob(**base))


def test_engine_adam_round_follows_the_rule():
    eng = _engine(server_optimizer="adam", server_lr=0.1)
    so = eng.server_opt
    start = eng.master.flat.clone()
    P = start.numel()
    assert so.m.shape == so.v.shape == (P,) and not so.m.any()
    v0 = so.v.clone()
    assert torch.equal(v0.cpu(), torch.full((P,), 1e-3 * 1e-3))
    eng.run_round(0)
    # single process: the accumulator still holds the round's delta
    delta = eng._delta
    assert float(delta.abs().max()) > 0
    ref = sr.reference("adam", start, delta, torch.zeros(P), v0, None,
                       sr.scalars(total_weight=8.0, sigma=0.0, lr=0.1,
                                  b1=0.9, b2=0.99, tau=1e-3))
    sr.assert_step_bounded("adam", eng.master.flat, so.m, so.v, ref, v0,
                           "engine.gpu.adam")
    assert so.steps == 1
    m1 = so.m.clone()
    eng.run_round(1)
    assert so.steps == 2 and not torch.equal(so.m, m1)


def test_engine_without_optimiser_is_apply_aggregate():
    from olearning_sim_amd.ops import fused
    eng = _engine()
    assert eng.server_opt is None
    want = eng.master.flat.clone()
    eng.run_round(0)
    fused.apply_aggregate([want], [eng._delta], 8.0)
    assert torch.equal(eng.master.flat, want)
