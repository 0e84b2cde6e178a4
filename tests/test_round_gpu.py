"""Whole rounds of LogicalEngine on the GPU, fp32, against the fp64
federation of round_ref.py: cohort rotation, offline and dropped clients,
tail padding, a round without weight, a round without clients, clipping,
noise and the server optimisers over five rounds, with the extension's
calls counted; the deferred aggregation path; interleaved evaluate
operators; resume from a checkpoint; and the same table once in bf16.
test_round_cpu.py proves that the comparison rejects an engine that gets
any of these wrong."""

import time

import pytest
import torch

import round_ref as rr

pytestmark = pytest.mark.gpu

COUNTED = ("server_opt_step", "client_delta_sqnorm", "clip_weights",
           "weighted_delta_accum_flat", "weighted_delta_accum_flat_dw",
           "fused_sgd_update_flat", "replicate")


class _CountingOps:
    """The extension namespace with a round's calls counted."""

    def __init__(self, ops):
        self._ops = ops
        self.calls = {name: 0 for name in COUNTED}

    def __getattr__(self, name):
        fn = getattr(self._ops, name)
        if name not in COUNTED:
            return fn

        def counted(*a, **kw):
            self.calls[name] += 1
            return fn(*a, **kw)
        return counted


@pytest.fixture(autouse=True)
def hip_ops_loaded():
    """No test of this module may pass on a torch fall-back."""
    from olearning_sim_amd.ops import fused
    fused.load_hip_ops(required=True)
    assert fused.hip_ops_available()


@pytest.fixture
def counting_ops(monkeypatch):
    from olearning_sim_amd.ops import fused
    proxy = _CountingOps(fused.load_hip_ops(required=True))
    monkeypatch.setattr(fused, "_HIP_OPS", proxy)
    return proxy


_DIRECT: dict = {}


def _direct(name, setting):
    """The direct fp32 GPU run of a case, made once and only read."""
    if (name, setting) not in _DIRECT:
        _DIRECT[(name, setting)] = rr.engine_run(name, setting, "cuda")
    return _DIRECT[(name, setting)]


def _equal_states(a, b):
    for t in ("flat", "m", "v"):
        if a[t] is None or b[t] is None:
            assert a[t] is None and b[t] is None, t
        else:
            assert a[t].is_cuda and torch.equal(a[t], b[t]), t
    assert a["steps"] == b["steps"]


@pytest.mark.parametrize("case", rr.CASES, ids=rr.case_id)
def test_gpu_rounds_match_the_fp64_federation(case, counting_ops):
    name, setting = case
    kind, _, clip, _ = rr._setting(setting)
    per_round = []

    def after_round(eng, r):
        torch.cuda.synchronize()
        per_round.append(dict(counting_ops.calls))

    t0 = time.perf_counter()
    run = rr.engine_run(name, setting, "cuda", after_round=after_round)
    print(f"engine[{name}.{setting}] {time.perf_counter() - t0:.3f} s")
    assert run["final"]["flat"].is_cuda
    rr.assert_round_bounded(name, setting, run, "cuda", what="gpu")

    # the HIP ops ran: per round the difference of the running counts
    P = len(rr.round_case(name)["gp0"])
    zero = {n: 0 for n in COUNTED}
    accum = "weighted_delta_accum_flat" + ("_dw" if clip else "")
    other = "weighted_delta_accum_flat" + ("" if clip else "_dw")
    for r, (before, after) in enumerate(zip([zero] + per_round, per_round)):
        got = {n: after[n] - before[n] for n in COUNTED}
        chunks = rr.CHUNKS_PER_ROUND[r]
        W = [5.0, 2.0, 0.0, 0.0, 4.0][r]
        assert got["server_opt_step"] == (1 if kind and W > 0 else 0), r
        # every parameter of both models has a gradient; the chunks of
        # the round in which everyone is dropped run like any other
        assert got["fused_sgd_update_flat"] == rr.STEPS * P * chunks, r
        assert got["client_delta_sqnorm"] == P * chunks, r
        assert got["clip_weights"] == (chunks if clip else 0), r
        assert got[accum] == P * chunks and got[other] == 0, r
        if chunks == 0:
            assert got == zero
        else:
            assert got["replicate"] > 0
    # round 2 (no weight) and round 3 (no clients) leave everything as it
    # was, bit for bit (round_exact checks the same; here in the open)
    states = run["starts"] + [run["final"]]
    _equal_states(states[2], states[3])
    _equal_states(states[3], states[4])


@pytest.mark.parametrize("case", rr.CASES, ids=rr.case_id)
def test_gpu_deferred_aggregation_equals_direct(case):
    """A 2-rank context without a process group: the all-reduce is the
    identity, and _pending_agg, the swap to the second delta buffer and
    the fold at the next master read run as they do on a 2-rank job."""
    name, setting = case
    seen = []

    def after_round(eng, r):
        seen.append((eng._pending_agg, eng._delta.data_ptr()))

    direct = _direct(name, setting)
    deferred = rr.engine_run(name, setting, "cuda:0", deferred=True,
                             after_round=after_round)
    assert deferred["eng"].ctx.enabled and len(seen) == rr.ROUNDS
    for r, (pending, ptr) in enumerate(seen):
        assert pending is not None and pending[0] is None
        assert pending[1].is_cuda and pending[1].data_ptr() != ptr
        assert pending[2:] == ([5.0, 2.0, 0.0, 0.0, 4.0][r], r)
    # "starts" is the state once the round before is folded in
    for a, b in zip(direct["starts"] + [direct["final"]],
                    deferred["starts"] + [deferred["final"]]):
        _equal_states(a, b)
    assert deferred["records"] == direct["records"]
    rr.assert_round_bounded(name, setting, deferred, "cuda",
                            what="gpu.deferred")


@pytest.mark.parametrize("setting", rr.SETTINGS)
def test_gpu_interleaved_evaluate(setting):
    """An evaluate operator after every train operator: eval_loss within
    tol of the fp64 forward of the reference master on the same held-out
    batch, eval_acc equal to it (round_failures asserts that no held-out
    row's top-2 logits lie within tol of each other)."""
    run = rr.engine_run("mlp", setting, "cuda", evaluate=True)
    ref = rr.round_reference("mlp", setting, "cuda")
    for rec, want in zip(run["records"], ref["rounds"]):
        assert 0 < rec["eval_loss"] and rec["eval_acc"] == want["eval_acc"]
    rr.assert_round_bounded("mlp", setting, run, "cuda", what="gpu.eval")
    if setting != "adam-noise":
        return
    deferred = rr.engine_run("mlp", setting, "cuda:0", deferred=True,
                             evaluate=True)
    # the evaluation reads the master: the pending round is folded first
    assert [(r["eval_loss"], r["eval_acc"]) for r in deferred["records"]] \
        == [(r["eval_loss"], r["eval_acc"]) for r in run["records"]]


@pytest.mark.parametrize("name", ["mlp", "lstm"])
def test_gpu_resume_continues_bit_for_bit(name, tmp_path):
    setting = "adam-noise"
    whole = _direct(name, setting)
    head = rr.engine_run(name, setting, "cuda", stop_after=1,
                         checkpoint_dir=str(tmp_path))
    assert len(head["records"]) == 2
    tail = rr.engine_run(name, setting, "cuda", resume=True,
                         checkpoint_dir=str(tmp_path))
    assert tail["first"] == 2 and len(tail["records"]) == 3
    # at 7 clients every accumulate is run-to-run identical
    _equal_states(head["final"], whole["starts"][2])
    for a, b in zip(tail["starts"] + [tail["final"]],
                    whole["starts"][2:] + [whole["final"]]):
        _equal_states(a, b)
    assert tail["final"]["steps"] == 3
    assert tail["applied"] == [(4, 4.0)] and head["applied"] == [(0, 5.0),
                                                                 (1, 2.0)]
    for got, want in zip(head["records"] + tail["records"],
                         whole["records"]):
        got = {k: v for k, v in got.items() if k != "checkpoint"}
        assert got == want


@pytest.mark.parametrize("name", ["mlp", "lstm"])
def test_gpu_bf16_rounds_keep_the_exact_parts(name):
    """bf16 is not compared with fp64 end to end (docs/TESTING.md).  The
    same table in bf16 must still reproduce every integer record field -
    ``clipped`` included, under round_ref.BF16_CLIP_GAP's condition on the
    reference - the applied weights, the step counts and the rounds that
    must not move."""
    setting = "adam-noise"
    run = rr.engine_run(name, setting, "cuda", dtype="bfloat16")
    assert run["eng"].trainer._cast_flat.dtype == torch.bfloat16
    rr.assert_bf16_exact(name, setting, run, "cuda")
    assert bool(torch.isfinite(run["final"]["flat"]).all())
    for r in rr.MOVING:
        assert run["records"][r]["update_norm_mean"] > 0
