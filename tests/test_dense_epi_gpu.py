"""The dense-layer epilogue kernels (ops/csrc/dense_epi.hip): each kernel
against fp64 on the exact bf16 tensors it reads, their writes, the route, and
BertLM on the fused route against the fp64 model.

Bounds (kb.bound; intrinsic=True where v_exp_f32 / v_rsq_f32 take part).
GELU, u = z + b formed once in fp32, A = |z| + |b|, Pa = (1 + |erf|) / 2 the
distribution function on absolute values, p the density:
y      u Phi(u): the rounding of u moves it by |gelu'| <= Pa + |u| p per unit
       of A, Phi is evaluated against Pa and the product rounds once more:
       scale A (Pa + |u| p), n = 1, one bf16 rounding.
dz     dy (Phi + u p): as above, and the rounding of u moves gelu' by
       |gelu''| = p |2 - u^2|: scale |dy| (Pa + |u| p + A p (2 + u^2)), n = 2.
db     sums N stored dz in fp32 (n = N), one bf16 rounding, and inherits the
       column sum of dz's bound.
LayerNorm, everything after s against kb.norm_math on the kernel's own s:
s      one rounding of a three-term fp32 sum: scale |z| + |b| + |res|, n = 2.
mean   an H-term fp32 sum: norm_math's mean_scale, n = H.
rstd   the variance is the mean of (s - mean)^2, H non-negative terms, so its
       summation error is relative to itself and d rstd = rstd^3 d var / 2
       <= rstd / 2 per unit; the error e_m of the mean enters only as e_m^2
       (the deviations sum to zero): scale rstd, n = H, extra rstd^3 e_m^2 / 2.
y, ds  norm_math's pre / dx and their scales, n = H, as for ops.layernorm.
dgamma sums N terms dy xhat in fp32 (n = N) and inherits the column sum of
       the terms' own H-term bound; dbeta sums N exact terms (n = N); db sums
       N stored ds (n = N) and inherits the column sum of ds's bound.
"""

import pytest
import torch

import kernel_bounds as kb

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
SENTINEL = 12345.678
PAD = 64
EPS = float(torch.tensor(1e-5, dtype=F32))
GELU_CASES = [(2, 4, 8), (3, 5, 24), (2, 70, 520), (1, 1, 3072)]
LN_CASES = [(2, 4, 8, 0.3), (2, 70, 72, 0.3), (2, 8, 520, 0.3),
            (1, 4, 1536, 0.3), (3, 36, 768, 0.3), (3, 8, 768, 8.0)]
_RUNS: dict = {}


@pytest.fixture(autouse=True)
def _fused_route(monkeypatch):
    monkeypatch.setenv("OLSIM_DENSE_EPI", "fused")


def _place(shape, dtype):
    """An output PAD elements into SENTINEL-filled storage, and the storage."""
    n = int(torch.Size(shape).numel())
    whole = torch.full((n + 2 * PAD,), SENTINEL, device="cuda", dtype=dtype)
    return whole[PAD:PAD + n].view(shape), whole


def _rand(gen, shape, std, mean=0.0):
    return (mean + std * torch.randn(shape, generator=gen)).to(BF16).cuda()


def _gelu_run(C, N, F):
    key = ("gelu", C, N, F)
    if key not in _RUNS:
        from olearning_sim_amd.ops import dense_epi
        gen = torch.Generator().manual_seed(C + 3 * N + 7 * F)
        z, b = _rand(gen, (C, N, F), 2.5), _rand(gen, (C, F), 0.5)
        dy = _rand(gen, (C, N, F), 0.1)
        out, whole = {}, {}
        for name, shape in [("y", z.shape), ("dz", z.shape), ("db", (1, C, F))]:
            out[name], whole[name] = _place(shape, BF16)
        dense_epi.bias_gelu_fwd(z, b, out=out["y"])
        dense_epi.bias_gelu_bwd(z, b, dy, dz=out["dz"], db=out["db"])
        again = dense_epi.bias_gelu_bwd(z, b, dy)
        torch.cuda.synchronize()
        _RUNS[key] = dict(out, whole=whole, z=z, b=b, dy=dy, again=again,
                          first=(out["dz"], out["db"]))
    return _RUNS[key]


def _ln_run(C, N, H, shift):
    key = ("ln", C, N, H, shift)
    if key not in _RUNS:
        from olearning_sim_amd.ops import dense_epi
        gen = torch.Generator().manual_seed(C + 3 * N + 7 * H)
        spread = 0.5 if shift == 8.0 else 2.0
        z, res = _rand(gen, (C, N, H), spread, shift), _rand(gen, (C, N, H), 1.0)
        b, beta = _rand(gen, (C, H), 0.5), _rand(gen, (C, H), 0.2)
        gamma = _rand(gen, (C, H), 0.5, 1.0)
        dy = _rand(gen, (C, N, H), 0.1)
        out, whole = {}, {}
        for name, shape, dt in [("y", z.shape, BF16), ("s", z.shape, BF16),
                                ("mean", (C, N), F32), ("rstd", (C, N), F32),
                                ("ds", z.shape, BF16), ("cols", (3, C, H), BF16)]:
            out[name], whole[name] = _place(shape, dt)
        dense_epi.brln_fwd(z, b, res, gamma, beta, EPS, **{
            k: out[k] for k in ("y", "s", "mean", "rstd")})
        args = (out["s"], dy, gamma, out["mean"], out["rstd"])
        dense_epi.brln_bwd(*args, ds=out["ds"], cols=out["cols"])
        again = dense_epi.brln_bwd(*args)
        torch.cuda.synchronize()
        _RUNS[key] = dict(out, whole=whole, z=z, b=b, res=res, gamma=gamma,
                          beta=beta, dy=dy, again=again,
                          first=(out["ds"], out["cols"]))
    return _RUNS[key]


@pytest.mark.parametrize("C,N,F", GELU_CASES)
def test_bias_gelu_against_fp64(C, N, F):
    r, up = _gelu_run(C, N, F), kb.upcast
    label = f"gelu.{C}.{N}.{F}"
    z, b, dy = up(r["z"]), up(r["b"]).unsqueeze(1), up(r["dy"])
    u, A = z + b, z.abs() + b.abs()
    erf = torch.erf(u * 0.5 ** 0.5)
    Phi, Pa = 0.5 * (1 + erf), 0.5 * (1 + erf.abs())
    p = torch.exp(-0.5 * u * u) / (2 * torch.pi) ** 0.5
    assert float(u.min()) < -3 or N * F < 64, "no GELU tail in the inputs"
    kb.assert_bounded(r["y"], u * Phi, A * (Pa + u.abs() * p), 1, BF16,
                      intrinsic=True, label=label + ".y")
    dz = dy * (Phi + u * p)
    dz_scale = dy.abs() * (Pa + u.abs() * p + A * p * (2 + u * u))
    kb.assert_bounded(r["dz"], dz, dz_scale, 2, BF16, intrinsic=True,
                      label=label + ".dz")
    e_dz = kb.bound(dz, dz_scale, 2, BF16, intrinsic=True)
    kb.assert_bounded(r["db"][0], dz.sum(dim=1), dz_scale.sum(dim=1), N, BF16,
                      label=label + ".db", extra=e_dz.sum(dim=1))


@pytest.mark.parametrize("C,N,H,shift", LN_CASES)
def test_bias_residual_layernorm_against_fp64(C, N, H, shift):
    r, up = _ln_run(C, N, H, shift), kb.upcast
    label = f"brln.{C}.{N}.{H}.{shift}"
    z, b, res = up(r["z"]), up(r["b"]).unsqueeze(1), up(r["res"])
    kb.assert_bounded(r["s"], z + b + res, z.abs() + b.abs() + res.abs(), 2,
                      BF16, label=label + ".s")
    m = kb.norm_math(up(r["s"]), up(r["gamma"]).unsqueeze(1),
                     up(r["beta"]).unsqueeze(1), (-1,), EPS, dy=up(r["dy"]))
    kb.assert_bounded(r["mean"].unsqueeze(2), m["mean"], m["mean_scale"], H,
                      F32, label=label + ".mean")
    e_m = kb.bound(m["mean"], m["mean_scale"], H, F32)
    kb.assert_bounded(r["rstd"].unsqueeze(2), m["rstd"], m["rstd"], H, F32,
                      intrinsic=True, label=label + ".rstd",
                      extra=0.5 * m["rstd"] ** 3 * e_m ** 2)
    kb.assert_bounded(r["y"], m["pre"], m["pre_scale"], H, BF16,
                      intrinsic=True, label=label + ".y")
    kb.assert_bounded(r["ds"], m["dx"], m["dx_scale"], H, BF16,
                      intrinsic=True, label=label + ".ds")
    dgamma, dbeta, db = r["cols"]
    e_gx = kb.bound(m["gx"], m["gx_scale"], H, F32, intrinsic=True)
    kb.assert_bounded(dgamma, m["gx"].sum(1), m["gx_scale"].sum(1), N, BF16,
                      label=label + ".dgamma", extra=e_gx.sum(1))
    kb.assert_bounded(dbeta, m["g"].sum(1), m["g"].abs().sum(1), N, BF16,
                      label=label + ".dbeta")
    e_ds = kb.bound(m["dx"], m["dx_scale"], H, BF16, intrinsic=True)
    kb.assert_bounded(db, m["dx"].sum(1), m["dx_scale"].sum(1), N, BF16,
                      label=label + ".db", extra=e_ds.sum(1))


@pytest.mark.parametrize("run,case", [(_gelu_run, c) for c in GELU_CASES]
                         + [(_ln_run, c) for c in LN_CASES], ids=str)
def test_writes_and_determinism(run, case):
    r = run(*case)
    for name, whole in r["whole"].items():
        sent = torch.full((PAD,), SENTINEL, device="cuda", dtype=whole.dtype)
        assert torch.equal(whole[:PAD], sent), (name, "head")
        assert torch.equal(whole[-PAD:], sent), (name, "tail")
        body = whole[PAD:-PAD]
        assert not bool((body == sent[0]).any()), (name, "element not written")
    for a, b in zip(r["first"], r["again"]):
        assert torch.equal(a, b), "the backward is not reproducible"


def test_one_gradient_for_z_and_res():
    from olearning_sim_amd.ops import bias_residual_layernorm
    r = _ln_run(*LN_CASES[1])
    z, res = (r[k].clone().requires_grad_(True) for k in ("z", "res"))
    y = bias_residual_layernorm(z, r["b"], res, r["gamma"], r["beta"], EPS)
    gz, gres = torch.autograd.grad(y, (z, res), r["dy"])
    assert gz.data_ptr() == gres.data_ptr()
    assert torch.equal(gz, r["ds"]) and torch.equal(y, r["y"])


def test_route(monkeypatch):
    from olearning_sim_amd import ops

    def route(W, ln=False, dtype=BF16, off=0, device="cuda", strided=False):
        z = torch.zeros(6 * W + off, device=device, dtype=dtype)[off:] \
            .view(2, 3, W)
        b = torch.zeros(2, W, device=device, dtype=dtype)
        res = torch.zeros(2, 3, 2 * W, device=device, dtype=dtype)[..., :W] \
            if strided else torch.zeros_like(z)
        return ops.dense_epi_route(z, b, res, b, b) if ln \
            else ops.dense_epi_route(z, b)

    assert {route(F) for _, _, F in GELU_CASES} == {"fused"}
    assert {route(H, ln=True) for _, _, H, _ in LN_CASES} == {"fused"}
    assert route(1544) == "fused" and route(1544, ln=True) == "torch"
    for kwargs in (dict(dtype=F32), dict(device="cpu"), dict(off=1)):
        assert route(16, **kwargs) == route(16, ln=True, **kwargs) == "torch"
    assert route(12) == route(12, ln=True) == "torch"
    assert route(16, ln=True, strided=True) == "torch"
    monkeypatch.setenv("OLSIM_DENSE_EPI", "torch")
    assert route(16) == route(16, ln=True) == "torch"


def test_bert_on_the_fused_route(monkeypatch):
    """Loss and every parameter gradient: the fused route's error against the
    fp64 model is at most twice the composed route's, plus one bf16 unit."""
    from olearning_sim_amd.models.bert import _TiedHeadCE
    from olearning_sim_amd.ops import dense_epi
    monkeypatch.setattr(_TiedHeadCE, "SLICE_V", 16)
    case = kb.model_case("bert")
    model, x, y = case["model"], case["x"].cuda(), case["y"].cuda()
    params = {k: v.to(BF16).cuda() for k, v in case["params"].items()}

    def errors(route):
        monkeypatch.setenv("OLSIM_DENSE_EPI", route)
        before = dense_epi.DENSE_EPI_CALLS
        loss, grads = kb.model_loss_and_grads(model, params, x, y)
        errs = {k: kb._rel_max(g, case["g64"][k]) for k, g in grads.items()}
        errs["loss"] = kb._rel_max(loss, case["loss64"])
        return dense_epi.DENSE_EPI_CALLS - before, errs

    calls_t, e_torch = errors("torch")
    calls_f, e_fused = errors("fused")
    # per layer three forward kernels, and per backward a kernel and the finish
    assert (calls_t, calls_f) == (0, model.layers * (3 + 3 * 2))
    for k in e_torch:
        print(f"bert[{k}] fused {e_fused[k]:.3e} torch {e_torch[k]:.3e}")
    bad = {k: (e_fused[k], e_torch[k]) for k in e_torch
           if not e_fused[k] <= 2 * e_torch[k] + kb.U_OUT[BF16]}
    assert not bad, bad
