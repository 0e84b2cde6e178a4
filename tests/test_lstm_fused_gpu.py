"""The fused LSTM recurrence (ops/csrc/lstm.hip): both kernels step by step
against fp64 from the tensors they stored (lstm_ref.py), the route, and
CharLSTM on the fused route against the same model in fp64."""

import pytest
import torch

import kernel_bounds as kb
import lstm_ref

pytestmark = pytest.mark.gpu

SENTINEL = 12345.678
PAD = 64
C = 3
# (H, B, L): every JT template, B masked and full, L without feedback, with
# the first feedback, and through both LDS buffer parities
CASES = [(64, 1, 1), (64, 5, 2), (64, 16, 5), (128, 5, 5), (128, 16, 1),
         (128, 1, 2), (192, 1, 5), (192, 16, 2), (192, 5, 1), (256, 5, 1),
         (256, 1, 2), (256, 16, 5)]
_RUNS: dict = {}


def _place(shape, dtype):
    """An uninitialised operand PAD elements into SENTINEL-filled storage."""
    n = int(torch.Size(shape).numel())
    whole = torch.full((n + 2 * PAD,), SENTINEL, device="cuda", dtype=dtype)
    return whole[PAD:PAD + n].view(shape), whole


def _run(H, B, L):
    """One forward and backward of the case, outputs inside sentinels."""
    key = (H, B, L)
    if key not in _RUNS:
        from olearning_sim_amd.ops import lstm
        gen = torch.Generator().manual_seed(H + 17 * B + L)
        xp = (2.0 * torch.randn(C, B, L, 4 * H, generator=gen)).bfloat16().cuda()
        w = ((torch.rand(C, H, 4 * H, generator=gen) * 2 - 1)
             / H ** 0.5).bfloat16().cuda()
        dhs = torch.randn(C, B, L, H, generator=gen).bfloat16().cuda()
        out, whole = {}, {}
        for name, mult, dt in (("hs", 1, torch.bfloat16),
                               ("gates", 4, torch.bfloat16),
                               ("cs", 1, torch.float32),
                               ("dgates", 4, torch.bfloat16)):
            out[name], whole[name] = _place((C, B, L, mult * H), dt)
        lstm.lstm_forward(xp, w, out["hs"], out["gates"], out["cs"])
        _, out["dw"] = lstm.lstm_backward(dhs, out["gates"], out["cs"],
                                          out["hs"], w, out["dgates"])
        torch.cuda.synchronize()
        _RUNS[key] = dict(out, xp=xp, w=w, dhs=dhs, whole=whole)
    return _RUNS[key]


@pytest.mark.parametrize("H,B,L", CASES)
def test_forward_steps_bounded(H, B, L):
    r = _run(H, B, L)
    lstm_ref.check_forward(r["xp"], r["w"], r["hs"], r["gates"], r["cs"],
                           f"lstm.fwd.H{H}.B{B}.L{L}")


@pytest.mark.parametrize("H,B,L", CASES)
def test_backward_steps_bounded(H, B, L):
    r = _run(H, B, L)
    lstm_ref.check_backward(r["dhs"], r["gates"], r["cs"], r["hs"], r["w"],
                            r["dgates"], r["dw"], f"lstm.bwd.H{H}.B{B}.L{L}")


@pytest.mark.parametrize("H,B,L", CASES)
def test_no_write_outside_the_outputs(H, B, L):
    for name, whole in _run(H, B, L)["whole"].items():
        sent = torch.full((PAD,), SENTINEL, device="cuda", dtype=whole.dtype)
        assert torch.equal(whole[:PAD], sent), (name, "head")
        assert torch.equal(whole[-PAD:], sent), (name, "tail")


def test_route():
    from olearning_sim_amd import ops

    def route(B, H, dtype=torch.bfloat16, off=0):
        xp = torch.zeros(2 * B * 3 * 4 * H + off, device="cuda",
                         dtype=dtype)[off:].view(2, B, 3, 4 * H)
        return ops.lstm_route(xp, torch.zeros(2, H, 4 * H, device="cuda",
                                              dtype=dtype))

    assert route(16, 64) == "fused"
    assert route(8, 16) == "torch"
    assert route(17, 64) == "torch"
    assert route(8, 320) == "torch"
    assert route(16, 64, torch.float32) == "torch"
    assert route(16, 64, off=1) == "torch"
    assert ops.lstm_route(torch.zeros(2, 16, 3, 256).bfloat16(),
                          torch.zeros(2, 64, 256).bfloat16()) == "torch"


def _rel_l2(got, ref):
    return float((kb.upcast(got) - ref).norm() / ref.norm())


def test_model_on_the_fused_route_against_fp64(monkeypatch):
    """Loss and every parameter gradient of a bf16 CharLSTM: the fused
    route's relative L2 error against fp64 is at most twice the torch
    route's own (OLSIM_LSTM=torch, same inputs)."""
    from olearning_sim_amd.models import build_model
    from olearning_sim_amd.ops import lstm
    model = build_model("lstm", vocab_size=30, embed=8, hidden=64, layers=2,
                        seq_len=5)
    gen = torch.Generator().manual_seed(3)
    params = {k: (v.unsqueeze(0).expand(C, *v.shape)
                  + 0.05 * torch.randn((C,) + v.shape, generator=gen)).bfloat16()
              for k, v in model.init_global(generator=gen).items()}
    x = torch.randint(0, 30, (C, 5, 5), generator=gen)
    y = torch.randint(0, 30, (C, 5, 5), generator=gen)

    p64 = {k: v.double().requires_grad_(True) for k, v in params.items()}
    loss64 = kb.ce_math(model.forward(p64, x).reshape(-1, 30),
                        y.reshape(-1))["loss"]
    ref = dict(zip(p64, torch.autograd.grad(loss64, list(p64.values()))))
    ref["loss"] = loss64.detach()

    def errs():
        loss, grads = kb.model_loss_and_grads(
            model, {k: v.cuda() for k, v in params.items()}, x.cuda(), y.cuda())
        return {k: _rel_l2(dict(grads, loss=loss)[k], ref[k]) for k in ref}

    before = lstm.LAYER_CALLS
    fused = errs()
    assert lstm.LAYER_CALLS - before == model.layers
    monkeypatch.setenv("OLSIM_LSTM", "torch")
    torch_route = errs()
    assert lstm.LAYER_CALLS - before == model.layers
    for k in ref:
        print(f"lstm model {k}: fused {fused[k]:.3e} torch {torch_route[k]:.3e}"
              f" ratio {fused[k] / torch_route[k]:.3f}")
    bad = {k: fused[k] / torch_route[k] for k in ref
           if not fused[k] <= 2 * torch_route[k]}
    assert not bad, bad
