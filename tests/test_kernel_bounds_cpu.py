"""The bound helper must accept an honest fp32 kernel and reject the
subtle bugs the GPU numerics tests exist to catch.

For each checked operation, at one small shape: a torch stand-in kernel
(bf16-rounded inputs, fp32 math, ONE rounding to the output dtype) has
to pass ``assert_bounded`` against the fp64 reference, and every mutant
has to fail it.  No GPU needed."""

import pytest
import torch

import kernel_bounds as kb
from kernel_bounds import assert_bounded, upcast

BF, F32 = torch.bfloat16, torch.float32


def _rejects(*args, **kw):
    with pytest.raises(AssertionError):
        assert_bounded(*args, **kw)


# -- the helper itself ------------------------------------------------------

def test_bound_terms_and_failure_report():
    ref = torch.tensor([1.0, -2.0, 0.0], dtype=torch.float64)
    scale = torch.tensor([1.0, 2.0, 0.5], dtype=torch.float64)
    b = kb.bound(ref, scale, 6, BF)
    want = 2.0 ** -8 * ref.abs() + 8 * 2.0 ** -23 * scale + 2.0 ** -126
    assert torch.equal(b, want)
    b = kb.bound(ref, scale, 6, F32, intrinsic=True)
    want = (2.0 ** -22 * ref.abs() + (8 * 2.0 ** -23 + 2.0 ** -16) * scale
            + 2.0 ** -126)
    assert torch.equal(b, want)
    b2 = kb.bound(ref, scale, 6, BF, roundings=2)
    assert torch.equal(b2 - kb.bound(ref, scale, 6, BF), 2.0 ** -8 * ref.abs())
    got = ref.clone()
    got[1] += 3 * float(kb.bound(ref, scale, 6, BF)[1])
    with pytest.raises(AssertionError) as e:
        assert_bounded(got, ref, scale, 6, BF, label="probe")
    msg = str(e.value)
    assert "index (1,)" in msg and "3.000 x bound" in msg
    # a where-mask excludes the element; a NaN never passes
    keep = torch.tensor([True, False, True])
    assert assert_bounded(got, ref, scale, 6, BF, where=keep) == 0.0
    got[0] = float("nan")
    _rejects(got, ref, scale, 6, BF)


def test_upcast_is_exact_copy_of_kernel_input():
    x = torch.randn(64).to(BF)
    u = upcast(x)
    assert u.dtype == torch.float64 and u.device.type == "cpu"
    assert torch.equal(u.to(BF), x)


# -- cross-entropy ----------------------------------------------------------

@pytest.mark.parametrize("dtype", [F32, BF])
def test_cross_entropy_emulation_passes_mutants_fail(dtype):
    g = torch.Generator().manual_seed(1)
    N, K = 256, 100
    logits = (torch.randn(N, K, generator=g) * 3).to(dtype)
    labels = torch.randint(0, K, (N,), generator=g)
    ref = kb.ce_math(upcast(logits), labels, upstream=3.0)

    def emu(mutant=None):
        r = kb.ce_math(logits.float(), labels, upstream=3.0, mutant=mutant)
        return r["grad"].to(dtype), r["loss"]

    grad, loss = emu()
    assert_bounded(grad, ref["grad"], ref["grad_scale"], K, dtype,
                   intrinsic=True, label="ce.grad")
    assert_bounded(loss, ref["loss"], ref["loss_scale"], K + N, F32,
                   intrinsic=True, label="ce.loss")
    for mutant in ("zero", "no_onehot"):
        _rejects(emu(mutant)[0], ref["grad"], ref["grad_scale"], K, dtype,
                 intrinsic=True)
        _rejects(emu(mutant)[0], ref["grad"], ref["grad_scale"], K, dtype,
                 intrinsic=True, roundings=2)
    # what the autograd path does: dlogits stored in the logits dtype,
    # then multiplied by the upstream gradient in that dtype again
    r1 = kb.ce_math(logits.float(), labels)
    twice = (r1["grad"].to(dtype).float() * 3.0).to(dtype)
    assert_bounded(twice, ref["grad"], ref["grad_scale"], K, dtype,
                   intrinsic=True, label="ce.grad.2x", roundings=2)
    if dtype == BF:         # one bf16 rounding is all that 2^-8 covers
        _rejects(twice, ref["grad"], ref["grad_scale"], K, dtype,
                 intrinsic=True)


# -- LayerNorm / GroupNorm --------------------------------------------------

def _norm_case(kind, dtype, shift=False):
    g = torch.Generator().manual_seed(9)
    if kind == "ln":
        C, N, H = 3, 8, 128
        x = torch.randn(C, N, H, generator=g) * 2 + 0.3
        gamma = torch.randn(C, 1, H, generator=g) * 0.5 + 1.0
        beta = torch.randn(C, 1, H, generator=g) * 0.2
        dims, n = (-1,), H
    else:
        C, G, cg, B, Hh, Ww = 2, 8, 2, 2, 4, 8
        x = torch.randn(C, G, cg, B, Hh, Ww, generator=g)
        gamma = 1 + 0.1 * torch.randn(C, G, cg, 1, 1, 1, generator=g)
        beta = 0.1 * torch.randn(C, G, cg, 1, 1, 1, generator=g)
        dims, n = (2, 4, 5), cg * Hh * Ww
    if shift:
        x = 8 + 0.5 * torch.randn(x.shape, generator=g)
    dy = torch.randn(x.shape, generator=g) * 0.1
    return [t.to(dtype) for t in (x, gamma, beta, dy)], dims, n


@pytest.mark.parametrize("kind", ["ln", "gn"])
@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("shift", [False, True])
def test_norm_emulation_passes_mutants_fail(kind, dtype, shift):
    (x, gamma, beta, dy), dims, n = _norm_case(kind, dtype, shift)
    ref = kb.norm_math(upcast(x), upcast(gamma), upcast(beta), dims, 1e-5,
                       dy=upcast(dy))

    def emu(mutant=None):
        return kb.norm_math(x.float(), gamma.float(), beta.float(), dims,
                            1e-5, dy=dy.float(), kernel_var=True,
                            mutant=mutant)

    e = emu()
    assert_bounded(e["pre"].to(dtype), ref["pre"], ref["pre_scale"], n,
                   dtype, intrinsic=True, label=f"{kind}.y")
    assert_bounded(e["dx"].to(dtype), ref["dx"], ref["dx_scale"], n, dtype,
                   intrinsic=True, label=f"{kind}.dx")
    assert_bounded(e["mean"], ref["mean"], ref["mean_scale"], n, F32,
                   label=f"{kind}.mean")
    assert_bounded(e["rstd"], ref["rstd"], ref["rstd_scale"], n, F32,
                   intrinsic=True, label=f"{kind}.rstd")
    if shift:
        return
    for mutant in ("no_mean", "no_xhat", "no_both"):
        _rejects(emu(mutant)["dx"].to(dtype), ref["dx"], ref["dx_scale"], n,
                 dtype, intrinsic=True)


# -- conv3x3 ----------------------------------------------------------------

def test_conv3x3_emulation_passes_mutants_fail():
    g = torch.Generator().manual_seed(2)
    C, IC, OC, B, H, W = 2, 16, 8, 2, 8, 8
    x = (torch.randn(C, IC, B, H, W, generator=g) * 0.5).to(BF)
    w = (torch.randn(C, OC, IC, 3, 3, generator=g) * 0.1).to(BF)
    dy = (torch.randn(C, OC, B, H, W, generator=g) * 0.1).to(BF)
    ref = kb.conv_ref(upcast(x), upcast(w), upcast(dy), 1, 1)
    nq = B * H * W

    def check(y, dx, dw):
        assert_bounded(y.to(BF), ref["y"], ref["y_scale"], IC * 9, BF,
                       label="conv3.y")
        assert_bounded(dx.to(BF), ref["dx"], ref["dx_scale"], OC * 9, BF,
                       label="conv3.dx")
        assert_bounded(dw.to(BF), ref["dw"], ref["dw_scale"], nq, BF,
                       label="conv3.dw")

    check(*kb.conv_all(x.float(), w.float(), dy.float(), 1, 1))

    x_drop = x.float().clone()
    x_drop[:, -1] = 0                       # last input channel dropped
    y_m = kb.conv_math(x_drop, w.float(), 1, 1)
    _rejects(y_m.to(BF), ref["y"], ref["y_scale"], IC * 9, BF)

    w_drop = w.float().clone()
    w_drop[..., 2, 0] = 0                   # one tap dropped
    y_m = kb.conv_math(x.float(), w_drop, 1, 1)
    _rejects(y_m.to(BF), ref["y"], ref["y_scale"], IC * 9, BF)

    # pipeline tail: the last 32 of the B*OH*OW reduction positions of
    # wgrad never accumulated
    dy_tail = dy.float().clone()
    dy_tail.view(C, OC, nq)[:, :, -32:] = 0
    _, _, dw_m = kb.conv_all(x.float(), w.float(), dy_tail, 1, 1)
    _rejects(dw_m.to(BF), ref["dw"], ref["dw_scale"], nq, BF)


# -- fused SGD / FedProx and delta accumulation -----------------------------

def _flat_layout(sizes, clients, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    P = sum(sizes)
    offs = [0]
    for s in sizes:
        offs.append(offs[-1] + s)
    master = torch.randn(P, generator=g).to(dtype)
    buf = torch.randn(clients * P, generator=g).to(dtype)
    grad = torch.randn(clients * P, generator=g).to(dtype)
    return buf, grad, master, offs


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("mu", [0.0, 0.3])
def test_fused_sgd_emulation_passes_lr_mutant_fails(dtype, mu):
    C = 5
    buf, grad, master, offs = _flat_layout([64, 15, 103], C, dtype, 0)
    ref, scale = kb.sgd_math(upcast(buf), upcast(grad), upcast(master), offs,
                             C, 0.1, mu)
    emu, _ = kb.sgd_math(buf.float(), grad.float(), master.float(), offs, C,
                         0.1, mu)
    assert_bounded(emu.to(dtype), ref, scale, 4, dtype, label="sgd")
    bad, _ = kb.sgd_math(buf.float(), grad.float(), master.float(), offs, C,
                         0.101, mu)          # lr off by 1 %
    _rejects(bad.to(dtype), ref, scale, 4, dtype)


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("C", [1, 5])
def test_delta_accum_emulation_passes_weight_mutant_fails(dtype, C):
    buf, _, master, offs = _flat_layout([64, 15, 103, 4096], C, dtype, 3)
    g = torch.Generator().manual_seed(4)
    w = torch.rand(C, generator=g)
    delta = torch.randn(master.numel(), generator=g)
    ref, scale, scale_h = kb.delta_math(
        upcast(delta), upcast(buf), upcast(master), upcast(w), offs, C)
    # master subtracted per client: the plain scale holds
    emu = kb.delta_math(delta.clone(), buf.float(), master.float(), w, offs,
                        C)[0]
    assert_bounded(emu, ref, scale, C + 1, F32, label="delta")
    # master hoisted out of the client loop (what aggregate.hip does):
    # judged against the abs-value evaluation of the hoisted expression
    emu_h = kb.delta_math(delta.clone(), buf.float(), master.float(), w,
                          offs, C, hoisted=True)[0]
    assert_bounded(emu_h, ref, scale_h, C + 1, F32, label="delta.hoisted")
    w_bad = w.clone()
    w_bad[C // 2] *= 1.01                   # one client weight off by 1 %
    bad = kb.delta_math(delta.clone(), buf.float(), master.float(), w_bad,
                        offs, C, hoisted=True)[0]
    _rejects(bad, ref, scale, C + 1, F32)
    _rejects(bad, ref, scale_h, C + 1, F32)
