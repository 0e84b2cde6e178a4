"""The fused causal attention for 129 <= L <= 512 (ops/csrc/attn_long.hip):
both kernels element-wise against fp64 (attn_long_ref.py), their writes, the
route, and a bf16 BertLM on the long route against the same model in fp64."""

import pytest
import torch

import attn_long_ref
import kernel_bounds as kb

pytestmark = pytest.mark.gpu

SENTINEL = 12345.678
PAD = 64
C, B = 1, 2
# (HD, heads, L): one row into the second block, a ragged second block with
# the head offset, two exact blocks, a third block of one row, ragged and no
# multiple of 16, a ragged last tile of the last block, the full range
CASES = [(64, 1, 129), (32, 3, 145), (64, 2, 256), (64, 1, 257),
         (32, 1, 300), (64, 3, 497), (64, 1, 512), (32, 2, 512)]
_RUNS: dict = {}


def _place(shape, dtype):
    """An uninitialised operand PAD elements into SENTINEL-filled storage."""
    n = int(torch.Size(shape).numel())
    whole = torch.full((n + 2 * PAD,), SENTINEL, device="cuda", dtype=dtype)
    return whole[PAD:PAD + n].view(shape), whole


def _run(HD, heads, L):
    """One forward and backward of the case, outputs inside sentinels."""
    key = (HD, heads, L)
    if key not in _RUNS:
        from olearning_sim_amd.ops import attn
        H = heads * HD
        gen = torch.Generator().manual_seed(HD + 17 * heads + L)
        qkv = torch.randn(C, B, L, 3 * H, generator=gen).bfloat16().cuda()
        datt = torch.randn(C, B, L, H, generator=gen).bfloat16().cuda()
        out, whole = {}, {}
        for name, shape, dt in (("att", (C, B, L, H), torch.bfloat16),
                                ("lse", (C * B, heads, L), torch.float32),
                                ("dsum", (C * B, heads, L), torch.float32),
                                ("dqkv", (C, B, L, 3 * H), torch.bfloat16)):
            out[name], whole[name] = _place(shape, dt)
        attn.attn_long_forward(qkv, heads, out["att"], out["lse"])
        attn.attn_long_backward(datt, qkv, out["att"], out["lse"], heads,
                                out["dqkv"], out["dsum"])
        torch.cuda.synchronize()
        _RUNS[key] = dict(out, qkv=qkv, datt=datt, whole=whole)
    return _RUNS[key]


@pytest.mark.parametrize("HD,heads,L", CASES)
def test_forward_and_backward_bounded(HD, heads, L):
    r = _run(HD, heads, L)
    label = f"attn_long.HD{HD}.h{heads}.L{L}"
    attn_long_ref.check_forward(r["qkv"], heads, r["att"], r["lse"], label)
    attn_long_ref.check_backward(r["qkv"], heads, r["att"], r["lse"],
                                 r["datt"], r["dqkv"], label)


@pytest.mark.parametrize("HD,heads,L", CASES)
def test_no_write_outside_the_outputs(HD, heads, L):
    r = _run(HD, heads, L)
    for name, whole in r["whole"].items():
        sent = torch.full((PAD,), SENTINEL, device="cuda", dtype=whole.dtype)
        assert torch.equal(whole[:PAD], sent), (name, "head")
        assert torch.equal(whole[-PAD:], sent), (name, "tail")
    sent = torch.tensor(SENTINEL, device="cuda", dtype=torch.bfloat16)
    assert not bool((r["dqkv"] == sent).any()), "dqkv element not written"


def test_route(monkeypatch):
    from olearning_sim_amd import ops
    from olearning_sim_amd.ops import attn

    def operand(L, HD, heads=2, dtype=torch.bfloat16, off=0, device="cuda"):
        w = 3 * heads * HD
        return torch.zeros(2 * L * w + off, device=device,
                           dtype=dtype)[off:].view(1, 2, L, w)

    def route(L, HD, **kw):
        return ops.attn_long_route(operand(L, HD, **kw), 2)

    assert [route(L, 64) for L in (128, 129, 512, 513)] == \
        ["torch", "long", "long", "torch"]
    assert [route(300, hd) for hd in (16, 32, 64, 128)] == \
        ["torch", "long", "long", "torch"]
    assert route(256, 64, dtype=torch.float32) == "torch"
    assert route(256, 64, off=1) == "torch"
    assert route(256, 64, device="cpu") == "torch"
    assert ops.attn_route(operand(129, 64), 2) == "torch"
    for L, HD in ((128, 64), (513, 64), (256, 16)):
        with pytest.raises(RuntimeError, match="not a long shape"):
            attn.attn_long_forward(operand(L, HD), 2)
    for switch in ("OLSIM_ATTN", "OLSIM_ATTN_LONG"):
        with monkeypatch.context() as mp:
            mp.setenv(switch, "torch")
            assert route(256, 64) == "torch"
    assert route(256, 64) == "long"


def _rel_l2(got, ref):
    return float((kb.upcast(got) - ref).norm() / ref.norm())


def test_model_on_the_long_route_against_fp64(monkeypatch):
    """Loss and every parameter gradient of a bf16 BertLM with HD = 64 and
    130 tokens: the long route's relative L2 error against fp64 is at most
    twice the torch route's own (OLSIM_ATTN=torch, same inputs)."""
    from olearning_sim_amd.models import build_model
    from olearning_sim_amd.ops import attn
    clients, V, L = 2, 40, 130
    model = build_model("bert", seq_len=L, vocab_size=V, hidden=128, layers=2,
                        heads=2)
    gen = torch.Generator().manual_seed(3)
    params = {k: (v.unsqueeze(0).expand(clients, *v.shape) + 0.05
                  * torch.randn((clients,) + v.shape, generator=gen)).bfloat16()
              for k, v in model.init_global(generator=gen).items()}
    x = torch.randint(0, V, (clients, 2, L), generator=gen)
    y = torch.randint(0, V, (clients, 2, L), generator=gen)

    p64 = {k: v.double().requires_grad_(True) for k, v in params.items()}
    loss64 = kb.ce_math(model.forward(p64, x).reshape(-1, V),
                        y.reshape(-1))["loss"]
    ref = dict(zip(p64, torch.autograd.grad(loss64, list(p64.values()))))
    ref["loss"] = loss64.detach()

    def errs():
        loss, grads = kb.model_loss_and_grads(
            model, {k: v.cuda() for k, v in params.items()}, x.cuda(), y.cuda())
        return {k: _rel_l2(dict(grads, loss=loss)[k], ref[k]) for k in ref}

    before = attn.ATTN_LONG_CALLS
    long_route = errs()
    assert attn.ATTN_LONG_CALLS - before == model.layers
    monkeypatch.setenv("OLSIM_ATTN", "torch")
    torch_route = errs()
    assert attn.ATTN_LONG_CALLS - before == model.layers
    for k in ref:
        print(f"bert model {k}: long {long_route[k]:.3e} torch "
              f"{torch_route[k]:.3e} ratio {long_route[k] / torch_route[k]:.3f}")
    bad = {k: long_route[k] / torch_route[k] for k in ref
           if not long_route[k] <= 2 * torch_route[k]}
    assert not bad, bad
