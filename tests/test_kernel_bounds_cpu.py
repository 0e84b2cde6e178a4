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


# -- per-client linear ------------------------------------------------------

def _linear_standin(x, w, b, dy, dtype, mutant=None):
    """fp32 math, rounded to ``dtype`` where _BLinearFn rounds: the bmm
    output, then (with a bias) the sum again."""
    r = kb.linear_math(x.float(), w.float(), None if b is None else b.float(),
                       dy.float(), mutant=mutant)
    y = r["xw"].to(dtype)
    if b is not None:
        y = (y.float() + b.float().unsqueeze(1)).to(dtype)
    return {"y": y, "dx": r["dx"].to(dtype), "dw": r["dw"].to(dtype),
            "db": r["db"].to(dtype)}


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("has_bias", [True, False])
def test_blinear_emulation_passes_mutants_fail(dtype, has_bias):
    g = torch.Generator().manual_seed(6)
    C, rows, fin, fout = 3, 8, 40, 24
    x = torch.randn(C, rows, fin, generator=g).to(dtype)
    w = (torch.randn(C, fin, fout, generator=g) * 0.2).to(dtype)
    b = torch.randn(C, fout, generator=g).to(dtype) if has_bias else None
    dy = (torch.randn(C, rows, fout, generator=g) * 0.1).to(dtype)
    ref = kb.linear_math(upcast(x), upcast(w),
                         None if b is None else upcast(b), upcast(dy))
    kb.assert_linear_bounded(_linear_standin(x, w, b, dy, dtype), ref, dtype,
                             has_bias)
    mutants = ["dw_untransposed", "dx_1pct"] + (["db_dropped"] if has_bias
                                                else [])
    for mutant in mutants:
        with pytest.raises(AssertionError):
            kb.assert_linear_bounded(
                _linear_standin(x, w, b, dy, dtype, mutant), ref, dtype,
                has_bias)


def test_blinear_bias_needs_its_own_rounding_term():
    """Where x@w and b cancel, the first rounding is large against |y|:
    the derived ``extra`` accepts the honest kernel, two roundings
    relative to |y| would not."""
    g = torch.Generator().manual_seed(8)
    C, rows, fin, fout = 2, 8, 16, 32
    x = torch.randn(C, rows, fin, generator=g).to(BF)
    w = torch.randn(C, fin, fout, generator=g).to(BF)
    xw = torch.bmm(x.float(), w.float())
    b = (-xw[:, 0] + 0.01).to(BF)            # row 0 of every client cancels
    dy = torch.randn(C, rows, fout, generator=g).to(BF)
    ref = kb.linear_math(upcast(x), upcast(w), upcast(b), upcast(dy))
    got = _linear_standin(x, w, b, dy, BF)
    kb.assert_linear_bounded(got, ref, BF, True)
    _rejects(got["y"], ref["y"], ref["y_scale"], fin, BF, roundings=2)


# -- transposes -------------------------------------------------------------

@pytest.mark.parametrize("N", [64, 90, 400, 218])
def test_thin_transpose_chunking_emulation_is_exact(N):
    """k_transpose_thin's decomposition: 128-column chunks, each written
    as out[n0:n0+nn, :M]."""
    x = torch.randn(3, 24, N).to(BF)
    out = torch.empty(3, N, 24, dtype=BF)
    for n0 in range(0, N, 128):
        nn = min(128, N - n0)
        out[:, n0:n0 + nn] = x[:, :, n0:n0 + nn].transpose(1, 2)
    assert torch.equal(out, x.transpose(1, 2).contiguous())


# -- 1x1 conv, stride 2 -----------------------------------------------------

def test_conv1x1_stride2_emulation_passes_odd_pixel_mutant_fails():
    g = torch.Generator().manual_seed(10)
    C, IC, OC, B, H, W = 2, 16, 32, 2, 8, 8
    x = (torch.randn(C, IC, B, H, W, generator=g) * 0.5).to(BF)
    w = (torch.randn(C, OC, IC, generator=g) * 0.1).to(BF)
    dy = (torch.randn(C, OC, B, 4, 4, generator=g) * 0.1).to(BF)
    ref = kb.conv_ref(upcast(x), upcast(w).view(C, OC, IC, 1, 1), upcast(dy),
                      2, 0)

    def emu(off):
        xs = x.float()[..., off::2, off::2].reshape(C, IC, B * 16)
        return torch.bmm(w.float(), xs).view(C, OC, B, 4, 4).to(BF)

    assert_bounded(emu(0), ref["y"], ref["y_scale"], IC, BF, label="conv1.y")
    _rejects(emu(1), ref["y"], ref["y_scale"], IC, BF)   # pixel (2i+1, 2j+1)


# -- tied head + cross-entropy ----------------------------------------------

def _tied_head_sliced(hs, tok, bias, labels, sv, dtype, mutant=None):
    """_TiedHeadCE's algorithm in fp32 torch with its roundings to
    ``dtype``: online-softmax forward over vocabulary slices, backward
    recomputing each slice.  Mutants: "skip_last" (last slice never
    visited), "wrong_slice" (the label's -1 lands in the next slice),
    "overwrite" (dhs = instead of dhs +=)."""
    C, N, H = hs.shape
    V = tok.shape[1]
    f = lambda t: t.float()
    rd = lambda t: t.to(dtype).float()
    starts = list(range(0, V, sv))
    if mutant == "skip_last":
        starts = starts[:-1]

    def logits_of(s0, s1):
        return rd(torch.bmm(f(hs), f(tok)[:, s0:s1].transpose(1, 2))) \
            + f(bias)[:, s0:s1].unsqueeze(1)

    m = torch.full((C, N), float("-inf"))
    l = torch.zeros(C, N)
    zy = torch.zeros(C, N)
    for s0 in starts:
        s1 = min(s0 + sv, V)
        z = logits_of(s0, s1)
        m_new = torch.maximum(m, z.max(dim=2).values)
        l = l * torch.exp(m - m_new) + torch.exp(z - m_new.unsqueeze(2)).sum(2)
        m = m_new
        sel = (labels >= s0) & (labels < s1)
        idx = (labels - s0).clamp(0, s1 - s0 - 1)
        zy = torch.where(sel, z.gather(2, idx.unsqueeze(2)).squeeze(2), zy)
    loss = (torch.log(l) + m - zy).mean()

    g = 1.0 / (C * N)
    lse = (m + torch.log(l)).unsqueeze(2)
    dhs = torch.zeros(C, N, H)
    dtok = torch.zeros(C, V, H)
    dbias = torch.zeros(C, V)
    for s0 in starts:
        s1 = min(s0 + sv, V)
        p = torch.exp(logits_of(s0, s1) - lse)
        lab = labels + sv if mutant == "wrong_slice" else labels
        lab = torch.where(lab >= V, lab - sv * len(starts), lab)
        sel = (lab >= s0) & (lab < s1)
        idx = (lab - s0).clamp(0, s1 - s0 - 1)
        p = p - torch.zeros_like(p).scatter_(2, idx.unsqueeze(2), 1.0) \
            * sel.unsqueeze(2)
        dl = rd(p * g)
        dbias[:, s0:s1] = rd(dl.sum(dim=1))
        part = rd(torch.bmm(dl, f(tok)[:, s0:s1]))
        dhs = part if mutant == "overwrite" else rd(dhs + part)
        dtok[:, s0:s1] = rd(torch.bmm(dl.transpose(1, 2), f(hs)))
    return {"loss": loss, "dhs": dhs.to(dtype), "dtok": dtok.to(dtype),
            "dbias": dbias.to(dtype)}


@pytest.mark.parametrize("dtype", [F32, BF])
def test_tied_head_emulation_passes_mutants_fail(dtype):
    g = torch.Generator().manual_seed(23)
    C, N, H, V, sv = 2, 8, 16, 40, 16
    hs = torch.randn(C, N, H, generator=g).to(dtype)
    tok = (torch.randn(C, V, H, generator=g) * 0.5).to(dtype)
    bias = (torch.randn(C, V, generator=g) * 0.5).to(dtype)
    labels = torch.tensor([[0, 15, 16, 31, 32, 39, 7, 20],
                           [39, 32, 31, 16, 15, 0, 33, 8]])
    ref = kb.tied_head_math(upcast(hs), upcast(tok), upcast(bias), labels, sv)
    args = (ref, upcast(hs), upcast(tok), dtype, sv)
    kb.assert_tied_head_bounded(
        _tied_head_sliced(hs, tok, bias, labels, sv, dtype), *args)
    # the model's own implementation, which also runs on the CPU
    from olearning_sim_amd.models.bert import _TiedHeadCE, tied_head_ce
    leaves = [t.clone().requires_grad_(True) for t in (hs, tok, bias)]
    old = _TiedHeadCE.SLICE_V
    _TiedHeadCE.SLICE_V = sv
    try:
        loss = tied_head_ce(*leaves, labels)
        loss.backward()
    finally:
        _TiedHeadCE.SLICE_V = old
    kb.assert_tied_head_bounded(
        {"loss": loss.detach(), "dhs": leaves[0].grad,
         "dtok": leaves[1].grad, "dbias": leaves[2].grad}, *args,
        label="tied.model")
    for mutant in ("skip_last", "wrong_slice", "overwrite"):
        with pytest.raises(AssertionError):
            kb.assert_tied_head_bounded(
                _tied_head_sliced(hs, tok, bias, labels, sv, dtype, mutant),
                *args)


# -- model gradients --------------------------------------------------------

class _BLinearStandIn(torch.autograd.Function):
    """_BLinearFn's forward and hand-written backward on the CPU, with an
    optional 1 % error in one of the three gradients."""
    mutant = None

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        ctx.has_bias = b is not None
        y = torch.bmm(x, w)
        return y if b is None else y + b.unsqueeze(1)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = dy.contiguous()
        k = {m: 1.01 if _BLinearStandIn.mutant == m else 1.0
             for m in ("dx", "dw", "db")}
        dx = k["dx"] * torch.bmm(dy, w.transpose(1, 2).contiguous())
        dw = k["dw"] * torch.bmm(x.transpose(1, 2).contiguous(), dy)
        db = k["db"] * dy.sum(dim=1) if ctx.has_bias else None
        return dx, dw, db


@pytest.mark.parametrize("name", ["mlp", "lstm", "bert"])
def test_model_gradient_check_accepts_standin_rejects_1pct(name, monkeypatch):
    import importlib
    case = kb.model_case(name)
    assert 0 < case["e_cpu32"] < 1e-5
    mod = importlib.import_module("olearning_sim_amd.models." + name)
    monkeypatch.setattr(
        mod, "blinear",
        lambda x, w, b=None: _BLinearStandIn.apply(x.contiguous(),
                                                   w.contiguous(), b))

    def run(mutant):
        monkeypatch.setattr(_BLinearStandIn, "mutant", mutant)
        loss, grads = kb.model_loss_and_grads(case["model"], case["params"],
                                              case["x"], case["y"])
        return kb.assert_model_bounded(name, loss, grads)

    run(None)
    for mutant in ("dx", "dw", "db"):
        with pytest.raises(AssertionError):
            run(mutant)


# -- the local trainer's chunk ----------------------------------------------

def _trainer_mutants(monkeypatch, model, C):
    """name -> context-free patcher of one of LocalTrainer's collaborators
    (ops.fused, the model); LocalTrainer itself is left alone."""
    from olearning_sim_amd.ops import fused
    real_sgd, real_accum = fused.fused_sgd_update, fused.weighted_delta_accum
    real_loss = model.loss

    def sgd(lr_scale=1.0, no_prox=False, skip_last=False):
        def patched(params, grads, lr, mu=0.0, global_params=None,
                    keep_wt=False):
            if skip_last and not keep_wt:       # keep_wt is False only there
                return
            real_sgd(params, grads, lr * lr_scale, 0.0 if no_prox else mu,
                     global_params, keep_wt)
        return lambda: monkeypatch.setattr(fused, "fused_sgd_update", patched)

    def accum(client, value=None, scale=1.0):
        def patched(delta, client_params, global_params, weights, wsum=None):
            w = weights.clone()
            w[client] = (w[client] if value is None else value) * scale
            real_accum(delta, client_params, global_params, w, wsum)
        return lambda: monkeypatch.setattr(fused, "weighted_delta_accum",
                                           patched)

    return {
        # gradient of the chunk mean: the trainer's "* C" has nothing to undo
        "chunk_mean": lambda: monkeypatch.setattr(
            model, "loss", lambda p, x, y: real_loss(p, x, y) / C,
            raising=False),
        "no_prox": sgd(no_prox=True),
        "skip_last_step": sgd(skip_last=True),
        "clip_ignored": lambda: monkeypatch.setattr(
            fused, "clip_weights",
            lambda sq, w, S: (w.float(), w.float().sum().reshape(1))),
        "zero_weight_counted": accum(1, value=1.0),
        "lr_1pct": sgd(lr_scale=1.01),
        "weight_1pct": accum(0, scale=1.01),
    }


@pytest.mark.parametrize("name", ["mlp", "lstm", "bert"])
def test_trainer_check_accepts_cpu_trainer_rejects_mutants(name, monkeypatch):
    case = kb.trainer_case(name)                 # before anything is patched
    assert 0 < case["e_cpu32"] and case["tol"] <= 0.05
    for clip in kb.TRAINER_CLIPS:
        kb.assert_trainer_bounded(name, *kb.trainer_run(name, clip),
                                  clip=clip)
        kb.assert_trainer_bounded(
            name, *kb.trainer_run(name, clip, chunks=((0, 1), (2,))),
            clip=clip)

    def rejected(mutant, clip):
        with monkeypatch.context() as mp:
            _trainer_mutants(mp, case["model"], case["C"])[mutant]()
            delta, sq = kb.trainer_run(name, clip)
        with pytest.raises(AssertionError):
            kb.assert_trainer_bounded(name, delta, sq, clip=clip)

    for mutant in ("chunk_mean", "no_prox", "skip_last_step",
                   "zero_weight_counted"):
        for clip in kb.TRAINER_CLIPS:
            rejected(mutant, clip)
    for clip in ("all", "one"):
        rejected("clip_ignored", clip)
        # the clip factor folded into the weights but not into their sum.
        # The CPU accumulate subtracts the master per client and never
        # reads wsum, so the mutant is formed from the honest result:
        # sum_c w_c s_c p_c - (sum_c w_c) p_global
        #   = delta - (sum_c w_c - sum_c w_c s_c) p_global
        ref = case["ref"][clip]
        delta, sq = kb.trainer_run(name, clip)
        lost = sum(kb.TRAINER_WEIGHTS) - float(ref["w_eff"].sum())
        assert lost > 0
        bad = {k: d.double() - lost * case["g64"][k] for k, d in delta.items()}
        with pytest.raises(AssertionError):
            kb.assert_trainer_bounded(name, bad, sq, clip=clip)
    if name == "mlp":
        # 1 % moves the result by about 5e-3 of max|delta|: far outside
        # MLP's tol, inside the LSTM's and BERT's
        for mutant in ("lr_1pct", "weight_1pct"):
            for clip in kb.TRAINER_CLIPS:
                rejected(mutant, clip)


def test_trainer_reference_and_fixed_data_are_what_they_say():
    """trainer_math on a model whose gradient is known in closed form, and
    FixedData's indexing."""

    class Quad:
        sequence_model = False

        def forward(self, params, x):          # logits = x * w, K = 2
            return x * params["w"].unsqueeze(1)

    # one row per client, label 0: loss = log(1 + exp((w1 - w0) x)) at
    # x = (1, 1); d/dw0 = -sigmoid(w1 - w0), d/dw1 = +sigmoid(w1 - w0)
    gp = {"w": torch.tensor([0.25, -0.5])}
    x = torch.ones(2, 1, 2)
    y = torch.zeros(2, 1, dtype=torch.int64)
    delta, sq, w_eff = kb.trainer_math(Quad(), gp, [(x, y)], [2.0, 1.0],
                                       lr=0.5, mu=0.5, steps=1, clip_norm=0.0)
    sg = float(torch.sigmoid(torch.tensor(-0.75, dtype=torch.float64)))
    step = 0.5 * sg                              # prox term is 0 at step 1
    want = torch.tensor([step, -step], dtype=torch.float64) * 3.0
    assert torch.allclose(delta["w"], want, rtol=1e-12, atol=0)
    assert torch.allclose(sq, torch.full((2,), 2 * step * step,
                                         dtype=torch.float64), rtol=1e-12)
    S = 0.5 * (2 * step * step) ** 0.5
    delta, sq, w_eff = kb.trainer_math(Quad(), gp, [(x, y)], [2.0, 1.0],
                                       lr=0.5, mu=0.5, steps=1, clip_norm=S)
    assert torch.allclose(w_eff, torch.tensor([1.0, 0.5], dtype=torch.float64),
                          rtol=1e-6)
    assert torch.allclose(delta["w"], want / 2, rtol=1e-6, atol=0)

    data = kb.FixedData([(torch.arange(12.0).view(3, 2, 2),
                          torch.arange(6).view(3, 2))])
    xs, ys = data.batch(torch.tensor([2, 0]), 0, 0, 2, torch.bfloat16)
    assert xs.dtype == torch.bfloat16 and xs[:, 0, 0].tolist() == [8.0, 0.0]
    assert ys.tolist() == [[4, 5], [0, 1]]


# -- operand layout of the bundled models -----------------------------------

@pytest.mark.parametrize("name", ["resnet18", "bert", "lstm", "mlp"])
def test_default_layouts_keep_vector_eligible_parameters_aligned(name):
    """replicate and the vector accumulate kernels read a parameter with
    numel % 8 == 0 as 16-byte packs, and refuse (clone, scalar kernel) a
    view that does not start on a 16-byte boundary.  In the default
    layouts every such parameter starts at a multiple of 8 elements of
    the flat master - 16 bytes in bf16 and fp16, 32 in fp32 - so the
    alignment guards leave these models on the kernels they ran before."""
    from olearning_sim_amd.models import build_model
    params = build_model(name).init_global(device="meta")
    off, eligible = 0, 0
    for key, v in params.items():
        n = v.numel()
        if n % 8 == 0:
            eligible += 1
            assert off % 8 == 0, f"{name}: {key} starts at element {off}"
        off += n
    assert eligible > 0
