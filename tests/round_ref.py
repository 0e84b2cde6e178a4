"""Whole federated rounds of ``LogicalEngine`` against an fp64 federation.

``federation_math`` is the reference: what a run of several rounds does to
the global model, the server optimiser's state and the round records, in
fp64 and with none of the engine's code (it uses the per-client trainer
reference of ``kernel_bounds`` and the optimiser rule of
``server_opt_ref``).  ``engine_run`` drives the engine over the same
pre-drawn data and behaviour masks (``RoundData``, ``ROUND_MASKS``), and
``assert_round_bounded`` compares the two under the trainer check's rule.

Per round r:

1. cohort = (r * cohort + arange(cohort)) % N
2. offline clients leave (they count as failed)
3. every other client trains alone from the current global parameters on
   its own rows (kernel_bounds._trainer_locals)
4. sq_c = ||p_c - p_global||^2, s_c = S / sqrt(sq_c) where sq_c > S^2
5. a dropped client's weight is 0, every other trained client's 1
6. W = sum of the weights
7. W > 0: g = delta / W + sigma * z, sigma = f32(noise_multiplier * S / W);
   plain rule x += g, otherwise server_opt_ref.step_math with v0 = tau^2
8. W = 0: master, m, v and the step count stay as they are

z is data: the caller draws it on the engine's device (``draw_z`` restates
the seed rule of ``LogicalEngine._noise``, which resume depends on).

Tolerance, per parameter tensor of the movement master_R - master_0, of m
and of v, per round's update_norm_mean and eval_loss:
e = max|got - ref| / max|ref| <= 64 * k * max(e_cpu32, 2^-22), e_cpu32 the
worst such figure of the CPU fp32 engine on the same case, measured at run
time (``round_baseline``, which asserts tol <= 0.05).  Integer record
fields, the weights the updates were applied with, the step count, the
rounds that must not move and eval_acc are exact.
"""

from __future__ import annotations

import torch

import kernel_bounds as kb
import server_opt_ref as sr

ROUNDS = 5
N = 7
COHORT = 5
CHUNK = 2
STEPS = 2
B = 8
MU = 0.5
EVAL_STEP = 10_000
EVAL_BATCH = 16
# job seed (initial master, noise) and the seed of the data table: chosen
# so that the conditions on the reference alone (round_reference) hold
SEED = 41
DATA_SEED = 17

_T, _F = True, False
# (offline, dropped) by cohort position
ROUND_MASKS = {
    # everyone trains: chunks 2 + 2 + 1 and one zero-weight repeat
    0: ([_F] * 5, [_F] * 5),
    # three train as [p0, p2], [p4, repeat]; p4 is dropped, so the second
    # chunk carries no weight in a round that moves
    1: ([_F, _T, _F, _T, _F], [_F, _F, _F, _F, _T]),
    # every client trains and is dropped: W = 0
    2: ([_F] * 5, [_T] * 5),
    # nobody is there: no chunk at all
    3: ([_T] * 5, [_F] * 5),
    # ordinary round, one dropped; starts from the master of round 1
    4: ([_F] * 5, [_F, _T, _F, _F, _F]),
}
MOVING = (0, 1, 4)
CHUNKS_PER_ROUND = (3, 2, 3, 0, 3)

OPTIMIZERS = {"plain": ("", 1.0), "momentum": ("momentum", 1.0),
              "adam": ("adam", 0.05)}
MODES = ("off", "clip", "noise")
SETTINGS = tuple(f"{o}-{m}" for o in OPTIMIZERS for m in MODES)
BETA1, BETA2, TAU = 0.9, 0.99, 1e-3
# LSTM runs each rule without clipping and with clipping and noise
CASES = [("mlp", s) for s in SETTINGS] + \
        [("lstm", s) for s in SETTINGS if not s.endswith("-clip")]

_CACHE: dict = {}
# label -> measured e_cpu32 of the case, next to kernel_bounds.HEADROOM's
# worst e / tol under the same label (an absolute error, not a ratio, so
# it does not go into that dict)
E_CPU32: dict = {}


def case_id(case):
    return f"{case[0]}-{case[1]}"


def draw_z(seed, round_idx, numel, device):
    """The round's standard normal tensor as LogicalEngine._noise's
    docstring fixes it: a generator on the engine's device seeded from
    (job.seed, round_idx) and not from the rank."""
    gen = torch.Generator(device=device)
    gen.manual_seed((seed * 1_000_003 + round_idx * 7919 + 0x5EED) % (2 ** 63))
    return torch.randn((numel,), generator=gen, device=device,
                       dtype=torch.float32)


class RoundData:
    """Stand-in for the engine's ``data``: table[(round_idx, step)] =
    (x [N, B, ...], y [N, B]) pre-drawn on the CPU over the whole
    population, the same numbers on every device; batch() returns the rows
    of client_ids on ``device``.  The held-out batch of evaluate_global is
    the entry (round_idx, EVAL_STEP), one row of EVAL_BATCH samples."""

    def __init__(self, table, device="cpu"):
        self.table = table
        self.device = torch.device(device)

    def batch(self, client_ids, round_idx, step, batch_size, dtype):
        x, y = self.table[(round_idx, step)]
        ids = client_ids.cpu()
        assert x.shape[1] == batch_size
        xs = x[ids].to(self.device)
        if xs.is_floating_point():
            xs = xs.to(dtype)
        return xs, y[ids].to(self.device)


def behavior(round_idx, cohort):
    assert cohort == COHORT
    off, drop = ROUND_MASKS[round_idx]
    return torch.tensor(off), torch.tensor(drop)


# ---------------------------------------------------------------------------
# the reference

def _flat(params):
    return torch.cat([v.reshape(-1) for v in params.values()])


def _unflat(flat, like):
    out, off = {}, 0
    for k, v in like.items():
        out[k] = flat[off:off + v.numel()].view(v.shape)
        off += v.numel()
    return out


def _eval_math(model, params, x, y):
    """fp64 loss (ce_math), accuracy and the smallest top-2 logit gap
    relative to max|logit| of ``params`` on one held-out batch
    (x [1, E, ...], y [1, E])."""
    with torch.no_grad():
        p = {k: v.unsqueeze(0) for k, v in params.items()}
        logits = model.forward(p, x.double() if x.is_floating_point() else x)
        K = logits.shape[-1]
        flat = logits.reshape(-1, K)
        labels = y.reshape(-1)
        loss = float(kb.ce_math(flat, labels)["loss"])
        acc = float((flat.argmax(-1) == labels).double().mean())
        top = flat.topk(2, dim=-1).values
        gap = float((top[:, 0] - top[:, 1]).min() / flat.abs().max())
    return loss, acc, gap


def federation_math(model, gp0, table, masks, rounds, clients, cohort, lr, mu,
                    steps, clip_norm=0.0, noise_multiplier=0.0, z=None,
                    optimizer="", server_lr=1.0, beta1=BETA1, beta2=BETA2,
                    tau=TAU, evaluate=False):
    """The federation in fp64 (module docstring).  gp0: the initial fp32
    global parameters; table: RoundData's; masks[r] = (offline, dropped) by
    cohort position; z[r]: flat fp32 standard normal tensor in the
    master's layout (None: no noise).  Returns the master before every
    round and after the last ("masters", R + 1 dicts), the optimiser's
    final "m", "v" (dicts, None without) and "steps", and per round the
    expected record fields, "total_weight", "clipped_any_weight" (what
    ``clipped`` would be if zero-weight rows of the chunks counted), the
    norms of the weighted clients and, with noise, "noise_share" =
    max|sigma z| / max|delta / W|."""
    S = kb._f32(clip_norm) if clip_norm > 0 else 0.0
    master = {k: v.detach().double().cpu().clone() for k, v in gp0.items()}
    P = sum(v.numel() for v in master.values())
    m = torch.zeros(P, dtype=torch.float64)
    v = None
    if optimizer in ("adagrad", "adam"):
        v = torch.full((P,), sr.f32(tau * tau), dtype=torch.float64)
    n_steps = 0
    masters = [master]
    out_rounds = []
    for r in range(rounds):
        ids = (r * cohort + torch.arange(cohort)) % clients
        off = torch.tensor(masks[r][0])
        drop = torch.tensor(masks[r][1])
        active = ids[~off]
        w = (~drop[~off]).double()
        W = float(w.sum())
        rec = {"success": int(active.numel()), "failed": int(off.sum()),
               "trained": int(active.numel()), "total_weight": W,
               "clipped": 0, "clipped_any_weight": 0,
               "update_norm_mean": None, "norms": None}
        if active.numel() > 0:
            batches = [(table[(r, s)][0][active], table[(r, s)][1][active])
                       for s in range(steps)]
            g64, finals = kb._trainer_locals(model, master, batches, lr, mu,
                                             steps)
            delta, sq, _ = kb._trainer_aggregate(g64, finals, w, S)
            live = w > 0
            if S > 0:
                rec["clipped"] = int((live & (sq > S * S)).sum())
                over = (sq > S * S).long()
                # the tail chunk repeats its last client
                pad = (-int(active.numel())) % CHUNK
                rec["clipped_any_weight"] = int(over.sum() + pad * over[-1])
            if W > 0:
                rec["update_norm_mean"] = float(sq[live].sqrt().mean())
                rec["norms"] = sq[live].sqrt()
        if W > 0:
            d = _flat(delta)
            zr, sigma = None, 0.0
            if noise_multiplier > 0:
                sigma = kb._f32(noise_multiplier * S / W)
                zr = z[r].detach().double().cpu()
                rec["noise_share"] = float((sigma * zr).abs().max()
                                           / (d / W).abs().max())
            x = _flat(master)
            if not optimizer:
                x = x + d / W
                if zr is not None:
                    x = x + sigma * zr
            else:
                sc = sr.scalars(total_weight=W, sigma=sigma, lr=server_lr,
                                b1=beta1, b2=beta2, tau=tau)
                st = sr.step_math(optimizer, x, d, m, v, zr, sc)
                x, m, v = st["x"], st["m"], st["v"]
                n_steps += 1
            master = {k: t.clone() for k, t in _unflat(x, master).items()}
        rec["steps"] = n_steps
        if evaluate:
            ex, ey = table[(r, EVAL_STEP)]
            rec["eval_loss"], rec["eval_acc"], rec["eval_gap"] = \
                _eval_math(model, master, ex, ey)
        masters.append(master)
        out_rounds.append(rec)
    like = masters[0]
    return {"masters": masters, "rounds": out_rounds, "steps": n_steps,
            "m": _unflat(m, like) if optimizer else None,
            "v": _unflat(v, like) if v is not None else None}


# ---------------------------------------------------------------------------
# the cases

def round_case(name):
    """Model, initial parameters, data table and clip norm of one model;
    built once."""
    key = ("case", name)
    if key in _CACHE:
        return _CACHE[key]
    from olearning_sim_amd.models import build_model
    kwargs = kb.MODEL_CASES[name][0]
    k = kb.MODEL_CASES[name][3]
    model = build_model(name, **kwargs)
    gp0 = model.init_global(device="cpu", dtype=torch.float32,
                            generator=torch.Generator().manual_seed(SEED))
    gen = torch.Generator().manual_seed(DATA_SEED)

    def draw(rows, batch):
        if model.sequence_model:
            V, L = model.vocab_size, model.seq_len
            return (torch.randint(0, V, (rows, batch, L), generator=gen),
                    torch.randint(0, V, (rows, batch, L), generator=gen))
        return (torch.randn((rows, batch) + tuple(model.input_shape),
                            generator=gen),
                torch.randint(0, model.num_classes, (rows, batch),
                              generator=gen))

    table = {}
    for r in range(ROUNDS):
        for s in range(STEPS):
            table[(r, s)] = draw(N, B)
        table[(r, EVAL_STEP)] = draw(1, EVAL_BATCH)
    lr = kb.TRAINER_LR[name]
    # S from the reference's round-0 norms (the same under every setting:
    # round 0 starts from gp0): half way between the second and the third
    # smallest, so round 0 clips three of its five clients
    first = federation_math(model, gp0, table, ROUND_MASKS, 1, N, COHORT, lr,
                            MU, STEPS)
    norms0 = first["rounds"][0]["norms"].sort().values
    S = kb._f32(0.5 * float(norms0[1] + norms0[2]))
    case = {"name": name, "model": model, "kwargs": kwargs, "k": k,
            "gp0": gp0, "table": table, "lr": lr, "S": S,
            "P": sum(v.numel() for v in gp0.values())}
    _CACHE[key] = case
    return case


def _setting(setting):
    opt, mode = setting.split("-")
    kind, server_lr = OPTIMIZERS[opt]
    return kind, server_lr, mode != "off", mode == "noise"


def round_reference(name, setting, device="cpu"):
    """federation_math of one case, z drawn on ``device``, with the
    conditions on the reference alone asserted; built once per case and
    device type."""
    case = round_case(name)
    kind, server_lr, clip, noise = _setting(setting)
    dev = torch.device(device)
    key = ("ref", name, setting, dev.type if noise else "any")
    if key in _CACHE:
        return _CACHE[key]
    S = case["S"] if clip else 0.0
    z = None
    if noise:
        z = [draw_z(SEED, r, case["P"], dev) for r in range(ROUNDS)]
    ref = federation_math(
        case["model"], case["gp0"], case["table"], ROUND_MASKS, ROUNDS, N,
        COHORT, case["lr"], MU, STEPS, clip_norm=S,
        noise_multiplier=1.0 if noise else 0.0, z=z, optimizer=kind,
        server_lr=server_lr, evaluate=not case["model"].sequence_model)
    label = f"{name}.{setting}"
    rounds = ref["rounds"]
    assert [rec["total_weight"] for rec in rounds] == [5.0, 2.0, 0.0, 0.0, 4.0]
    for k_ in case["gp0"]:
        move = ref["masters"][-1][k_] - ref["masters"][0][k_]
        assert float(move.abs().max()) > 0, f"{label}: {k_} does not move"
    for r in (2, 3):
        assert ref["masters"][r + 1] is ref["masters"][r]
    if clip:
        subset = 0
        for r in MOVING:
            norms = rounds[r]["norms"]
            # fp32 must not be able to flip a clip decision
            gap = ((norms - S).abs() / S).min()
            assert float(gap) > 0.01, (label, r, norms.tolist(), S)
            subset += 0 < rounds[r]["clipped"] < norms.numel()
        assert subset > 0, f"{label}: no round clips a strict subset"
        # a counted zero-weight client must show in ``clipped``
        assert any(rec["clipped_any_weight"] != rec["clipped"]
                   for rec in rounds), label
    if noise:
        # a missing noise term must not pass for rounding
        for r in MOVING:
            assert rounds[r]["noise_share"] >= 0.1, (label, r, rounds[r])
    _CACHE[key] = ref
    return ref


# ---------------------------------------------------------------------------
# the engine under test

def _state(eng):
    so = eng.server_opt
    return {"flat": eng.master.flat.detach().clone(),
            "m": so.m.detach().clone() if so is not None else None,
            "v": (so.v.detach().clone()
                  if so is not None and so.v is not None else None),
            "steps": so.steps if so is not None else 0}


def engine_run(name, setting, device="cpu", deferred=False, dtype="float32",
               evaluate=False, mutate=None, checkpoint_dir="", resume=False,
               stop_after=None, after_round=None):
    """LogicalEngine over the case's table, round by round (run() would
    stop at the first round with a failed client).  deferred: a 2-rank
    DistContext without a process group, so the all-reduce is the identity
    and the round's update waits in _pending_agg until the master is next
    read.  mutate(eng) runs after the data is swapped in.  Returns the
    records, the (round, total_weight) pairs _apply_update was called
    with, the state at every begin_round ("starts": master, m, v, steps
    once the round before is folded in) and after the last fold
    ("final")."""
    from olearning_sim_amd.engine.job import EngineJob
    from olearning_sim_amd.engine.round_loop import LogicalEngine
    from olearning_sim_amd.parallel.dist import DistContext
    case = round_case(name)
    kind, server_lr, clip, noise = _setting(setting)
    model = case["model"]
    ops = [("train", "train")] + ([("eval", "evaluate")] if evaluate else [])
    job = EngineJob(
        task_id="round_" + name, model_name=name,
        model_kwargs=dict(case["kwargs"]), clients=N, cohort_size=COHORT,
        rounds=ROUNDS, local_steps=STEPS, batch_size=B, lr=case["lr"],
        prox_mu=MU, clip_norm=case["S"] if clip else 0.0,
        noise_multiplier=1.0 if noise else 0.0, update_norm_stats=True,
        server_optimizer=kind, server_lr=server_lr, server_beta1=BETA1,
        server_beta2=BETA2, server_tau=TAU, dtype=dtype, device=device,
        chunk_clients=CHUNK, seed=SEED, operators=ops,
        eval_batch=EVAL_BATCH, dynamic_num=N,
        vocab_size=model.vocab_size if model.sequence_model else 0,
        seq_len=model.seq_len if model.sequence_model else 0,
        checkpoint_dir=checkpoint_dir, save_every_round=bool(checkpoint_dir),
        resume=resume)
    ctx = DistContext(world_size=2, device=device) if deferred else None
    eng = LogicalEngine(job, dist_ctx=ctx, behavior=behavior)
    eng.data = eng.trainer.data = RoundData(case["table"], eng.device)

    starts, applied = [], []
    real_begin, real_apply = eng.trainer.begin_round, eng._apply_update

    def begin_round():
        starts.append(_state(eng))
        real_begin()

    def apply_update(delta, total_weight, round_idx):
        applied.append((round_idx, float(total_weight)))
        real_apply(delta, total_weight, round_idx)

    eng.trainer.begin_round = begin_round
    eng._apply_update = apply_update
    # after the two recorders: a mutant that wraps _apply_update hands its
    # own weight on to the recorder
    if mutate is not None:
        mutate(eng)
    master0 = eng.master.state_dict()
    records = []
    first = eng.start_round
    last = ROUNDS if stop_after is None else stop_after + 1
    for r in range(first, last):
        records.append(eng.run_round(r))
        if after_round is not None:
            after_round(eng, r)
    eng._finish_aggregate()
    return {"eng": eng, "first": first, "records": records,
            "applied": applied, "starts": starts, "final": _state(eng),
            "master0": master0}


# ---------------------------------------------------------------------------
# the comparison

def _rel(got, ref):
    return float((got.detach().double().cpu() - ref).abs().max()
                 / ref.abs().max())


def round_errs(name, run, ref):
    """label -> e = max|got - ref| / max|ref| of a full run (rounds 0 to
    ROUNDS - 1) against the reference."""
    case = round_case(name)
    like = case["gp0"]
    errs = {}
    got_R = _unflat(run["final"]["flat"], like)
    for k, g0 in like.items():
        move = got_R[k].detach().double().cpu() - g0.double()
        errs["move." + k] = _rel(move, ref["masters"][-1][k]
                                 - ref["masters"][0][k])
    for name_ in ("m", "v"):
        if ref[name_] is None:
            continue
        if run["final"][name_] is None:
            # state the rule carries and the engine does not hold
            errs[f"{name_}.missing"] = float("inf")
            continue
        got = _unflat(run["final"][name_], like)
        for k in like:
            errs[f"{name_}.{k}"] = _rel(got[k], ref[name_][k])
    for rec, want in zip(run["records"], ref["rounds"]):
        r = rec["round"]
        if want["update_norm_mean"] is not None \
                and rec.get("update_norm_mean") is not None:
            errs[f"norm.r{r}"] = abs(rec["update_norm_mean"]
                                     - want["update_norm_mean"]) \
                / want["update_norm_mean"]
        if "eval_loss" in rec:
            errs[f"eval_loss.r{r}"] = abs(rec["eval_loss"]
                                          - want["eval_loss"]) \
                / abs(want["eval_loss"])
    for k, e in errs.items():
        assert e == e, f"{k} is not a number"
    return errs


def round_exact(name, run, ref):
    """Labels of the exact expectations a full run misses: the integer
    record fields, where update_norm_mean is None, the weights the updates
    were applied with, the optimiser's step count before every round and
    at the end, the rounds that must leave master, m and v bit for bit as
    they were, the initial master, eval_acc."""
    case = round_case(name)
    bad = []
    if run["first"] != 0 or len(run["records"]) != ROUNDS:
        return ["rounds"]
    for k, g0 in case["gp0"].items():
        if not torch.equal(run["master0"][k].cpu(), g0):
            bad.append("master0." + k)
    for rec, want in zip(run["records"], ref["rounds"]):
        r = rec["round"]
        for field in ("success", "failed", "trained", "clipped"):
            if rec[field] != want[field] \
                    or not isinstance(rec[field], int):
                bad.append(f"{field}.r{r}")
        if (rec["update_norm_mean"] is None) \
                != (want["update_norm_mean"] is None):
            bad.append(f"norm_none.r{r}")
        if "eval_acc" in rec and rec["eval_acc"] != want["eval_acc"]:
            bad.append(f"eval_acc.r{r}")
    want_applied = [(r, rec["total_weight"])
                    for r, rec in enumerate(ref["rounds"])
                    if rec["total_weight"] > 0]
    if run["applied"] != want_applied:
        bad.append("total_weight")
    states = run["starts"] + [run["final"]]
    if len(states) != ROUNDS + 1:
        return bad + ["begin_round"]
    steps = [0] + [rec["steps"] for rec in ref["rounds"]]
    if ref["m"] is not None and [s["steps"] for s in states] != steps:
        bad.append("steps")
    for r in (2, 3):
        for t in ("flat", "m", "v"):
            a, b = states[r][t], states[r + 1][t]
            if a is not None and not torch.equal(a, b):
                bad.append(f"nomove.{t}.r{r}")
    return bad


def round_tol(name, e_cpu32):
    k = kb.MODEL_CASES[name][3]
    return (kb.U_INTRINSIC / kb.U_OUT[torch.float32]) * k \
        * max(e_cpu32, kb.U_OUT[torch.float32])


def round_baseline(name, setting):
    """e_cpu32 and tol of one case: the CPU fp32 engine, direct path,
    against the reference with z drawn on the CPU; built once.  The CPU
    engine must meet every exact expectation itself."""
    key = ("base", name, setting)
    if key in _CACHE:
        return _CACHE[key]
    case = round_case(name)
    ref = round_reference(name, setting, "cpu")
    run = engine_run(name, setting, "cpu",
                     evaluate=not case["model"].sequence_model)
    bad = round_exact(name, run, ref)
    assert not bad, f"{name}.{setting}: CPU fp32 engine misses {bad}"
    e_cpu32 = max(round_errs(name, run, ref).values())
    tol = round_tol(name, e_cpu32)
    assert tol <= 0.05, \
        f"{name}.{setting}: e_cpu32 {e_cpu32:.2e} gives tol {tol:.2e}"
    base = {"e_cpu32": e_cpu32, "tol": tol, "run": run}
    _CACHE[key] = base
    return base


def round_failures(name, setting, run, device="cpu"):
    """Every expectation a full run misses, as labels: round_exact's, and
    "bound.<label>" for every figure of round_errs beyond tol.  Also
    returns the worst e / tol."""
    base = round_baseline(name, setting)
    ref = round_reference(name, setting, device)
    bad = round_exact(name, run, ref)
    if any("eval_loss" in rec for rec in run["records"]):
        # a held-out row whose top-2 logits lie within tol of each other
        # would leave eval_acc to rounding
        for r, rec in enumerate(ref["rounds"]):
            assert rec["eval_gap"] > base["tol"], (name, setting, r, rec)
    errs = round_errs(name, run, ref)
    bad += ["bound." + k for k, e in errs.items() if not e <= base["tol"]]
    ratio = max(e for e in errs.values()) / base["tol"]
    return bad, ratio


# Smallest distance of a weighted client's fp64 norm from S at which a
# bf16 run is held to the fp64 clip count: two bf16 output units (0.78 %),
# one for the bf16 cast of the master the clients start from and one for
# the bf16 replicas the norm is taken from.  The element errors are of
# either sign and enter the norm in quadrature, so the norm itself moves
# by much less than one unit (the CPU bf16 trainer's update_norm_mean lies
# 0.3 % from fp64); the margin is reasoning about the format, not a bound
# proven for every input, and a bf16 count that differs is a finding.
BF16_CLIP_GAP = 2 * kb.U_OUT[torch.bfloat16]


def assert_bf16_exact(name, setting, run, device="cpu"):
    """A bf16 run of the table reproduces every exact expectation,
    ``clipped`` included; first the condition on the reference that lets
    bf16 norms decide the clip count as fp64 does."""
    ref = round_reference(name, setting, device)
    S = round_case(name)["S"]
    for r in MOVING:
        norms = ref["rounds"][r]["norms"]
        gap = float(((norms - S).abs() / S).min())
        assert gap > BF16_CLIP_GAP, (name, setting, r, norms.tolist(), S)
    for rec, want in zip(run["records"], ref["rounds"]):
        print(f"bf16[{name}.{setting}] round {rec['round']}: clipped "
              f"{rec['clipped']} (fp64 {want['clipped']}), norm mean "
              f"{rec['update_norm_mean']} (fp64 {want['update_norm_mean']})")
    bad = round_exact(name, run, ref)
    assert not bad, f"{name}.{setting}.bf16: {bad}"


def assert_round_bounded(name, setting, run, device="cpu", what="direct"):
    """A full fp32 run within tol of federation_math and exact where it
    must be; returns the worst e / tol."""
    base = round_baseline(name, setting)
    bad, ratio = round_failures(name, setting, run, device)
    label = f"round.{name}.{setting}"
    kb.HEADROOM[label] = max(kb.HEADROOM.get(label, 0.0), ratio)
    E_CPU32[label] = base["e_cpu32"]
    print(f"round[{name}.{setting}.{what}] e_cpu32 = {base['e_cpu32']:.2e}, "
          f"tol = {base['tol']:.2e}, worst e/tol = {ratio:.4f}")
    assert not bad, f"{name}.{setting}.{what}: tol {base['tol']:.2e}: {bad}"
    return ratio
