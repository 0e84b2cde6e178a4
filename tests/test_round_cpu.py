"""The round check of round_ref.py is sharp: the CPU fp32 engine passes
every case on the direct and on the deferred aggregation path, and an
engine with one of the faults a round can have fails, at every setting the
fault applies to and with the label of the check meant for it.  The faults
are patched onto the engine object; nothing under olearning_sim_amd/ is
edited."""

import pytest
import torch

import round_ref as rr


@pytest.mark.parametrize("case", rr.CASES, ids=rr.case_id)
def test_cpu_engine_matches_the_fp64_federation(case):
    name, setting = case
    base = rr.round_baseline(name, setting)      # runs the direct engine
    assert 0 < base["e_cpu32"] and base["tol"] <= 0.05
    evaluate = name == "mlp"
    direct = base["run"]
    rr.assert_round_bounded(name, setting, direct)
    deferred = rr.engine_run(name, setting, deferred=True, evaluate=evaluate)
    assert deferred["eng"].ctx.enabled
    rr.assert_round_bounded(name, setting, deferred, what="deferred")
    # the same arithmetic in the same order: the deferral changes nothing
    for a, b in zip(direct["starts"] + [direct["final"]],
                    deferred["starts"] + [deferred["final"]]):
        for t in ("flat", "m", "v"):
            assert (a[t] is None and b[t] is None) or torch.equal(a[t], b[t])


def test_deferred_round_waits_in_the_other_buffer():
    """The deferred path does defer: after a round with weight the update
    is pending, the master has not moved and the accumulator has been
    swapped; the next master read folds it in."""
    seen = []

    def after_round(eng, r):
        seen.append((eng._pending_agg, eng._delta.data_ptr(),
                     eng.master.flat.clone()))

    run = rr.engine_run("mlp", "momentum-clip", deferred=True,
                        after_round=after_round)
    for r, (pending, ptr, flat) in enumerate(seen):
        assert pending is not None and pending[0] is None
        assert pending[2:] == ([5.0, 2.0, 0.0, 0.0, 4.0][r], r)
        assert pending[1].data_ptr() != ptr
        assert torch.equal(flat, run["starts"][r]["flat"])
    assert not torch.equal(run["final"]["flat"], seen[-1][2])


# ---------------------------------------------------------------------------
# mutants: name -> (settings it applies to, label prefixes that must fail,
# install(eng, mp) on the engine object[, before(mp) on a class])

def _wrap(obj, attr, make):
    real = getattr(obj, attr)
    setattr(obj, attr, make(real))


def _no_rotation(eng, mp):
    _wrap(eng, "select_cohort", lambda real: lambda r: real(0))


def _offline_trained(eng, mp):
    eng.behavior = lambda r, c: (torch.zeros(c, dtype=torch.bool),
                                 rr.behavior(r, c)[1])


def _dropped_counted(eng, mp):
    def make(real):
        def apply(delta, W, r):
            real(delta, W + sum(rr.ROUND_MASKS[r][1]), r)
        return apply
    _wrap(eng, "_apply_update", make)


def _chunk_weights(change):
    def install(eng, mp):
        def make(real):
            def train_chunk(cid, w, r, delta, wsum=None):
                w = change(cid, w.clone())
                return real(cid, w, r, delta, wsum=float(w.sum()))
            return train_chunk
        _wrap(eng.trainer, "train_chunk", make)
    return install


def _pad_weighted(cid, w):
    # cohort ids are distinct: a repeated id is the tail padding
    if int(cid[-1]) == int(cid[-2]):
        w[-1] = 1.0
    return w


def _weight_1pct(cid, w):
    w[0] *= 1.01
    return w


def _stale_cast(mp):
    # on the class and before the engine exists: engine_run's recorder
    # then calls through to it and only the cast goes missing
    from olearning_sim_amd.engine.local_train import LocalTrainer
    real = LocalTrainer.begin_round

    def begin_round(self):
        if self._cast_flat is None:
            real(self)
            # a cast to bf16 is a copy; in fp32 .to() returns the master
            # itself, which cannot go stale: take the copy here
            self._cast_flat = self._cast_flat.clone()

    mp.setattr(LocalTrainer, "begin_round", begin_round)


def _update_without_weight(eng, mp):
    # the W = 0 round applies its (zero) delta all the same, with the
    # weight clamped to 1 as a division guard would
    def make(real):
        def op_train(r, name="train"):
            rec = real(r, name)
            if r == 2:
                eng._finish_aggregate()
                zero = torch.zeros_like(eng.master.flat)
                eng._apply_update(zero, 1.0, r)
            return rec
        return op_train
    _wrap(eng, "_op_train", make)


def _sigma_per_chunk(eng, mp):
    _wrap(eng, "_noise",
          lambda real: lambda r, W: real(r, min(W, float(rr.CHUNK))))


def _noise_after_step(eng, mp):
    def make(real):
        def step(master, delta, W, noise=None, sigma=0.0):
            real(master, delta, W)
            if noise is not None:
                master.add_(noise, alpha=sigma)
        return step
    _wrap(eng.server_opt, "step", make)


def _seed_without_round(eng, mp):
    _wrap(eng, "_noise", lambda real: lambda r, W: real(0, W))


def _clipped_counts_all(eng, mp):
    def make(real):
        def counts(chunks):
            out = real(chunks)
            sq = torch.cat([c[0] for c in chunks])
            S = torch.tensor(eng.job.clip_norm, dtype=torch.float32)
            out[0] = float((sq > S * S).sum())
            return out
        return counts
    _wrap(eng, "_update_norm_counts", make)


def _server_lr_1pct(eng, mp):
    eng.server_opt.lr *= 1.01


def _no_fold_before_training(eng, mp):
    def make(real):
        def op_train(r, name="train"):
            eng._finish_aggregate = lambda: None
            try:
                return real(r, name)
            finally:
                del eng._finish_aggregate
        return op_train
    _wrap(eng, "_op_train", make)


_ALL = rr.SETTINGS
_CLIP = tuple(s for s in _ALL if not s.endswith("-off"))
_NOISE = tuple(s for s in _ALL if s.endswith("-noise"))
_OPT = tuple(s for s in _ALL if not s.startswith("plain"))
_OPT_NOISE = tuple(s for s in _OPT if s.endswith("-noise"))

MUTANTS = {
    "no_rotation": (_ALL, ("bound.move",), _no_rotation),
    "offline_trained": (_ALL, ("bound.move", "nomove.flat.r3"),
                        _offline_trained),
    "dropped_counted": (_ALL, ("total_weight", "bound.move"),
                        _dropped_counted),
    "pad_weighted": (_ALL, ("bound.move",), _chunk_weights(_pad_weighted)),
    "stale_cast": (_ALL, ("bound.move",), None, _stale_cast),
    # plain rule without noise: the zero delta moves nothing, the applied
    # weights alone show it; with noise the master moves; with an
    # optimiser the state decays and the step is counted
    "update_without_weight": (_ALL, ("total_weight",),
                              _update_without_weight),
    "noise_without_weight": (_NOISE, ("nomove.flat.r2",),
                             _update_without_weight),
    "step_without_weight": (_OPT, ("steps", "nomove.flat.r2", "nomove.m.r2"),
                            _update_without_weight),
    "sigma_per_chunk": (_NOISE, ("bound.move",), _sigma_per_chunk),
    "noise_after_step": (_OPT_NOISE, ("bound.m.",), _noise_after_step),
    "seed_without_round": (_NOISE, ("bound.move",), _seed_without_round),
    "clipped_counts_all": (_CLIP, ("clipped.r",), _clipped_counts_all),
    "server_lr_1pct": (_OPT, ("bound.move",), _server_lr_1pct),
    "weight_1pct": (_ALL, ("bound.move",), _chunk_weights(_weight_1pct)),
}
# 1 % moves the result by parts in a thousand: far outside the MLP's tol,
# inside the LSTM's
MLP_ONLY = ("server_lr_1pct", "weight_1pct")


def _mutant_cases():
    for mutant in MUTANTS:
        yield "mlp", mutant
        if mutant not in MLP_ONLY:
            yield "lstm", mutant


@pytest.mark.parametrize("name,mutant", list(_mutant_cases()),
                         ids=lambda v: v)
def test_round_check_rejects_the_mutant(name, mutant, monkeypatch):
    settings, labels, install, before = (MUTANTS[mutant] + (None,))[:4]
    ran = 0
    for case_name, setting in rr.CASES:
        if case_name != name or setting not in settings:
            continue
        rr.round_baseline(name, setting)         # before anything is patched
        with monkeypatch.context() as mp:
            if before is not None:
                before(mp)
            run = rr.engine_run(
                name, setting,
                mutate=install and (lambda eng: install(eng, mp)))
        bad, _ = rr.round_failures(name, setting, run)
        for label in labels:
            assert any(b.startswith(label) for b in bad), \
                f"{name}.{setting}: {mutant} not caught by {label}*: {bad}"
        ran += 1
    assert ran > 0


@pytest.mark.parametrize("name", ["mlp", "lstm"])
def test_deferred_round_lost_without_the_fold_before_training(name,
                                                              monkeypatch):
    """On the deferred path the update of round r is applied where the
    master is next read.  Without that read at the start of the next
    training operator, the next round trains from the old master and its
    own pending update replaces the waiting one."""
    for case_name, setting in rr.CASES:
        if case_name != name:
            continue
        run = rr.engine_run(
            name, setting, deferred=True,
            mutate=lambda eng: _no_fold_before_training(eng, monkeypatch))
        bad, _ = rr.round_failures(name, setting, run)
        assert "total_weight" in bad and any(
            b.startswith("bound.move") for b in bad), (setting, bad)
