"""sgd_conv3_wt (the SGD update that also rewrites the dgrad's flipped-
transposed weight copy) and the trainer path that keeps such copies.

Everything is compared bit for bit: the kernel's update is k_sgd_plain's
expression on the same operands, the copy is data movement, and with the
copies the backward runs the same forward kernel on the same bytes as
the per-call repack (tests/test_conv_dgrad_wt_gpu.py)."""

import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
# (C, OC, IC), as tests/test_conv_wflip_gpu.py
CASES = [(1, 32, 32), (3, 64, 64), (2, 32, 96), (2, 96, 32), (2, 128, 64)]
ENV_VARS = ("OLSIM_CONV", "OLSIM_CONV_V", "OLSIM_CONV_DW64", "OLSIM_CONV_DW8",
            "OLSIM_CONV_NMAJOR", "OLSIM_DGRAD_WT", "OLSIM_GN_PAD")


@pytest.fixture(scope="module")
def ops():
    from olearning_sim_amd.ops import load_hip_ops
    return load_hip_ops(required=True)


@pytest.fixture(autouse=True)
def _no_env(monkeypatch):
    for var in ENV_VARS:
        monkeypatch.delenv(var, raising=False)


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("case", CASES, ids=str)
def test_sgd_conv3_wt_matches_plain_update_and_wflip(ops, case):
    from olearning_sim_amd.ops.fused import fused_sgd_update
    C, OC, IC = case
    g = torch.Generator().manual_seed(sum(case))
    w = (torch.randn(C, OC, IC, 3, 3, generator=g) * 0.1).to(BF).cuda()
    grad = (torch.randn(C, OC, IC, 3, 3, generator=g) * 0.3).to(BF).cuda()
    lr = 0.05
    w_ref = w.clone()
    fused_sgd_update([w_ref], [grad], lr=lr)
    wt = torch.full((C, IC, OC, 3, 3), float("nan"), dtype=BF, device="cuda")
    ops.sgd_conv3_wt(w, grad, wt, lr)
    torch.cuda.synchronize()
    assert torch.equal(_bits(w), _bits(w_ref))
    assert not torch.equal(w, grad)             # it did move
    assert torch.equal(_bits(wt), _bits(ops.conv3x3_wflip(w)))


def test_sgd_conv3_wt_rejects_mismatched_operands(ops):
    w = torch.zeros(2, 32, 64, 3, 3, dtype=BF, device="cuda")
    with pytest.raises(RuntimeError):          # wt not [C, IC, OC, 3, 3]
        ops.sgd_conv3_wt(w, torch.zeros_like(w), torch.zeros_like(w), 0.1)
    with pytest.raises(RuntimeError):          # g of another shape
        ops.sgd_conv3_wt(w, torch.zeros(2, 32, 32, 3, 3, dtype=BF,
                                        device="cuda"),
                         torch.zeros(2, 64, 32, 3, 3, dtype=BF,
                                     device="cuda"), 0.1)


_REAL = {}      # the unpatched functions, whatever a previous call patched


def _train_once(ops, monkeypatch, local_steps=3, batch_size=2):
    """One LocalTrainer.train_chunk on ResNet18(width 0.5), C=2: replicas
    after the call, delta_flat and a dict of counts: wt copies attached,
    conv3x3_wflip calls, held copies a backward or an update found live."""
    from olearning_sim_amd.models import build_model
    from olearning_sim_amd.engine import local_train
    from olearning_sim_amd.engine.client_manager import FlatParams
    from olearning_sim_amd.engine.data import SyntheticFederatedData
    from olearning_sim_amd.ops import conv as conv_mod
    m = build_model("resnet18", num_classes=100, width_mult=0.5)
    gen = torch.Generator().manual_seed(0)
    master = FlatParams({k: v.cuda()
                         for k, v in m.init_global(generator=gen).items()})
    data = SyntheticFederatedData(clients=8, num_classes=100,
                                  input_shape=m.input_shape, seed=3,
                                  device="cuda")
    trainer = local_train.LocalTrainer(
        m, master, data, lr=0.05, prox_mu=0.0, local_steps=local_steps,
        batch_size=batch_size, dtype=BF, report_loss=False)
    kept = {}
    real_rep = _REAL.setdefault("rep", local_train.replicate_params)
    monkeypatch.setattr(
        local_train, "replicate_params",
        lambda cast, C: kept.setdefault("params", real_rep(cast, C)))
    attached = []
    real_attach = _REAL.setdefault("attach", conv_mod.attach_wt)
    monkeypatch.setattr(conv_mod, "attach_wt",
                        lambda w, wt: (attached.append(1),
                                       real_attach(w, wt))[1])
    live = []
    real_live = _REAL.setdefault("live", conv_mod._live_wt)

    def counted_live(held, w):
        wt = real_live(held, w)
        if wt is not None:
            live.append(1)
        return wt
    monkeypatch.setattr(conv_mod, "_live_wt", counted_live)
    flips = []
    real_flip = _REAL.setdefault("flip", ops.conv3x3_wflip)
    monkeypatch.setattr(ops, "conv3x3_wflip",
                        lambda w: (flips.append(1), real_flip(w))[1])
    trainer.begin_round()
    delta = master.zeros_like_flat()
    trainer.train_chunk(torch.tensor([1, 5], device="cuda"),
                        torch.tensor([1.0, 2.0], device="cuda"), 0, delta,
                        wsum=3.0)
    torch.cuda.synchronize()
    params = kept["params"]
    assert all(getattr(p, "_olsim_wt", None) is None for p in params.values())
    counts = dict(attached=len(attached), flips=len(flips), live=len(live))
    return {k: v.detach() for k, v in params.items()}, delta, counts


def test_trainer_with_held_wt_equals_dgrad_path(ops, monkeypatch):
    """Default (copies held across the local steps) and OLSIM_DGRAD_WT=
    repack against OLSIM_DGRAD_WT=0 (conv3x3_dgrad_p everywhere).  At this
    size the GroupNorm atomics are bit-stable (tests/test_gn_pad_gpu.py
    compares whole-model gradients exactly), so replicas and delta are
    too.  Equal results cannot tell a held copy from a quiet repack, so
    the calls are counted: 13 stride-1 3x3 weights have a dgrad."""
    monkeypatch.setenv("OLSIM_DGRAD_WT", "0")
    rep0, delta0, n0 = _train_once(ops, monkeypatch)
    assert n0 == dict(attached=0, flips=0, live=0)
    monkeypatch.setenv("OLSIM_DGRAD_WT", "repack")
    rep2, delta2, n2 = _train_once(ops, monkeypatch)
    # one repack per weight per backward, nothing held
    assert n2 == dict(attached=0, flips=13 * 3, live=0)
    monkeypatch.delenv("OLSIM_DGRAD_WT")
    rep1, delta1, n1 = _train_once(ops, monkeypatch)
    # attached from the master at step 1 and by the update after steps 1
    # and 2, not after 3; the only repacks are the 13 of the master; every
    # backward (13 x 3) and every keeping update (13 x 2) found its copy
    assert n1 == dict(attached=13 * 3, flips=13, live=13 * 3 + 13 * 2)
    for rep, delta in ((rep1, delta1), (rep2, delta2)):
        for k in rep0:
            assert torch.equal(rep[k], rep0[k]), k
        assert torch.equal(delta, delta0)


def test_trainer_holds_no_copy_the_backward_would_not_read(ops, monkeypatch):
    """B = 1: the 4x4 stage has B*H*W = 16, outside conv3x3_v6_ok, so its
    three weights get no copy; the other ten do."""
    assert not ops.conv3x3_v6_ok(256, 256, 1, 4, 4, 1)
    assert ops.conv3x3_v6_ok(128, 128, 1, 8, 8, 1)
    monkeypatch.setenv("OLSIM_DGRAD_WT", "0")
    rep0, delta0, _ = _train_once(ops, monkeypatch, 2, batch_size=1)
    monkeypatch.delenv("OLSIM_DGRAD_WT")
    rep1, delta1, n1 = _train_once(ops, monkeypatch, 2, batch_size=1)
    assert n1 == dict(attached=10 * 2, flips=10, live=10 * 2 + 10)
    for k in rep0:
        assert torch.equal(rep1[k], rep0[k]), k
    assert torch.equal(delta1, delta0)


def test_stale_wt_is_not_used(ops):
    """A copy attached to w must not survive a plain update of w."""
    from olearning_sim_amd.ops.conv import attach_wt, client_conv3x3
    from olearning_sim_amd.ops.fused import fused_sgd_update
    C, IC, OC, B, H, W = 2, 32, 64, 2, 8, 8
    g = torch.Generator().manual_seed(21)
    x = (torch.randn(C, IC, B, H, W, generator=g) * 0.5).to(BF).cuda()
    dy = (torch.randn(C, OC, B, H, W, generator=g) * 0.1).to(BF).cuda()
    grad = (torch.randn(C, OC, IC, 3, 3, generator=g) * 0.3).to(BF).cuda()
    w = (torch.randn(C, OC, IC, 3, 3, generator=g) * 0.1).to(BF).cuda()
    w.requires_grad_(True)
    attach_wt(w, ops.conv3x3_wflip(w.detach()))
    old = w.detach().clone()
    with torch.no_grad():
        fused_sgd_update([w], [grad], lr=0.5)            # plain path
    assert getattr(w, "_olsim_wt", None) is None
    assert not torch.equal(w.detach(), old)
    xg = x.clone().requires_grad_(True)
    client_conv3x3(xg, w, 1).backward(dy)
    torch.cuda.synchronize()
    ref = ops.conv3x3_dgrad_p(ops.pad2d(dy, 1), w.detach(), H, W, 1)
    assert torch.equal(xg.grad, ref)

    # a holder picked up in the forward and dropped before the backward:
    # the copy is overwritten to show that it is not read
    from olearning_sim_amd.ops.conv import drop_wt
    wt = ops.conv3x3_wflip(w.detach())
    attach_wt(w, wt)
    xg = x.clone().requires_grad_(True)
    y = client_conv3x3(xg, w, 1)
    drop_wt(w)
    wt.zero_()
    y.backward(dy)
    torch.cuda.synchronize()
    assert torch.equal(xg.grad, ref)

    # the same when the writer is an in-place torch op nobody told about
    attach_wt(w, ops.conv3x3_wflip(w.detach()))
    with torch.no_grad():
        w.mul_(0.5)
    xg = x.clone().requires_grad_(True)
    client_conv3x3(xg, w, 1).backward(dy)
    torch.cuda.synchronize()
    ref = ops.conv3x3_dgrad_p(ops.pad2d(dy, 1), w.detach(), H, W, 1)
    assert torch.equal(xg.grad, ref)
