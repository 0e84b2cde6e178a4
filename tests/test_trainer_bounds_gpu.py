"""LocalTrainer.train_chunk on the GPU, fp32, against the per-client fp64
reference of kernel_bounds.trainer_math: the loss * C scaling,
replicate_params, the list-form fused SGD / FedProx update against views
of the flat cast, the multi-step loop, client_delta_sqnorm, clip_weights
and the list-form accumulate into views of the flat delta.  The tolerance
comes from the CPU fp32 trainer's own error (kernel_bounds.trainer_case);
the CPU file proves that it rejects a wrong scaling by C, a dropped prox
term, a skipped step, a clip factor missing from the weight sum, an
ignored clip and a counted zero-weight client."""

import pytest
import torch

import kernel_bounds as kb

pytestmark = pytest.mark.gpu

COUNTED = ("fused_sgd_update_flat", "weighted_delta_accum_flat",
           "weighted_delta_accum_flat_dw", "client_delta_sqnorm",
           "clip_weights", "replicate")


class _CountingOps:
    """The extension namespace with the trainer tail's calls counted."""

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


@pytest.fixture
def counting_ops(monkeypatch):
    from olearning_sim_amd.ops import fused
    proxy = _CountingOps(fused.load_hip_ops(required=True))
    monkeypatch.setattr(fused, "_HIP_OPS", proxy)
    return proxy


@pytest.mark.parametrize("chunks", [((0, 1, 2),), ((0, 1), (2,))],
                         ids=["one_chunk", "two_chunks"])
@pytest.mark.parametrize("clip", kb.TRAINER_CLIPS)
@pytest.mark.parametrize("name", ["mlp", "lstm", "bert"])
def test_train_chunk_fp32_matches_fp64(name, clip, chunks, counting_ops,
                                       monkeypatch):
    if name == "bert":
        # several vocabulary slices, as in the model-gradient test
        from olearning_sim_amd.models.bert import _TiedHeadCE
        monkeypatch.setattr(_TiedHeadCE, "SLICE_V", 16)
    case = kb.trainer_case(name)
    delta, sq = kb.trainer_run(name, clip, device="cuda", chunks=chunks)
    assert all(d.is_cuda for d in delta.values())
    kb.assert_trainer_bounded(name, delta, sq, clip=clip)

    # the HIP ops ran, once per parameter (every parameter of these three
    # models has a gradient) per step and chunk
    P, n = len(case["gp"]), len(chunks)
    calls = counting_ops.calls
    assert calls["fused_sgd_update_flat"] == kb.TRAINER_STEPS * P * n
    assert calls["client_delta_sqnorm"] == P * n
    clipped = clip != "off"
    assert calls["clip_weights"] == (n if clipped else 0)
    assert calls["weighted_delta_accum_flat_dw"] == (P * n if clipped else 0)
    assert calls["weighted_delta_accum_flat"] == (0 if clipped else P * n)
    # fp32: 16 bytes are 4 elements
    vec = sum(v.numel() % 8 == 0 and off % 4 == 0
              for v, off in zip(case["gp"].values(), _offsets(case["gp"])))
    assert calls["replicate"] == vec * n and vec > 0


def _offsets(params):
    off = 0
    for v in params.values():
        yield off
        off += v.numel()
