"""conv3x3 (every kernel family and dispatch branch), conv5x5 and the
2x2 max-pool against fp64 references with the derived bounds of
tests/kernel_bounds.py.  Each conv3x3 case asserts the family the
dispatcher takes and the kernel, with its template arguments, of all
three directions; each conv5x5 case the route of all three directions.
A silent change of route or of a threshold inside a family fails here."""

import pytest
import torch

import kernel_bounds as kb
from kernel_bounds import assert_bounded, upcast

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


@pytest.fixture(scope="module", autouse=True)
def _require_ext():
    from olearning_sim_amd.ops import load_hip_ops
    load_hip_ops(required=True)


_REF_CACHE: dict = {}


def _conv3_case(shape):
    """Inputs and fp64 reference for (C, IC, OC, B, H, W, stride);
    computed once and shared between the tests that use the shape."""
    if shape not in _REF_CACHE:
        C, IC, OC, B, H, W, s = shape
        g = torch.Generator().manual_seed(hash(shape) % (2 ** 31))
        OH, OW = (H + s - 1) // s, (W + s - 1) // s
        x = (torch.randn(C, IC, B, H, W, generator=g) * 0.5).to(BF)
        w = (torch.randn(C, OC, IC, 3, 3, generator=g) * 0.1).to(BF)
        dy = (torch.randn(C, OC, B, OH, OW, generator=g) * 0.1).to(BF)
        ref = kb.conv_ref(upcast(x), upcast(w), upcast(dy), s, 1)
        _REF_CACHE[shape] = (x, w, dy, ref)
    return _REF_CACHE[shape]


def _check_conv3x3(shape, v6, tag, routes, forced_v5=False):
    """routes: the (fwd, dgrad, wgrad) kernels, as ops.conv3x3_route
    spells them, that the shape reaches under the environment the caller
    has set.  forced_v5: OLSIM_CONV_V=5 is set, which ops.conv3x3_v6_ok
    (the shape predicate) ignores; the dispatcher's own _v6_ok must then
    say v5 for a shape of the v6 family."""
    from olearning_sim_amd.ops.conv import client_conv3x3, _v6_ok
    from olearning_sim_amd.ops.fused import load_hip_ops
    ops = load_hip_ops(required=True)
    C, IC, OC, B, H, W, s = shape
    assert bool(ops.conv3x3_v6_ok(IC, OC, B, H, W, s)) == v6, \
        f"{shape}: expected the {'v6' if v6 else 'v5'} family"
    got = tuple(ops.conv3x3_route(d, IC, OC, B, H, W, s)
                for d in ("fwd", "dgrad", "wgrad"))
    assert got == tuple(routes), f"{shape}: routes {got}, expected {routes}"
    x, w, dy, ref = _conv3_case(shape)
    xg = x.cuda().requires_grad_(True)
    wg = w.cuda().requires_grad_(True)
    assert _v6_ok(ops, xg, wg, s) == (v6 and not forced_v5), \
        f"{shape}: dispatcher takes the wrong family"
    y = client_conv3x3(xg, wg, s)
    y.backward(dy.cuda())
    OH, OW = y.shape[-2:]
    assert_bounded(y, ref["y"], ref["y_scale"], IC * 9, BF,
                   label=tag + ".fwd")
    assert_bounded(xg.grad, ref["dx"], ref["dx_scale"], OC * 9, BF,
                   label=tag + ".dgrad")
    assert_bounded(wg.grad, ref["dw"], ref["dw_scale"], B * OH * OW, BF,
                   label=tag + ".wgrad")


# The expected routes below were read off the launchers' branches by hand
# (fwd_v6/v7<LG_OW,STRIDE>, dgrad_v6/v7/s2<LG_OW> with LG_OW = log2(OW)
# clamped to the instantiated range), not produced by conv3x3_route.

# (C, IC, OC, B, H, W, stride) of the v6 padded family -> (fwd, dgrad,
# wgrad) with no variable set
V6_ROUTES = {
    # the benchmark's stage 0
    (1, 64, 64, 1, 32, 32, 1): ("fwd_v7<5,1>", "dgrad_v6<4>", "wgrad_v8"),
    # non-square planes
    (2, 64, 64, 2, 8, 16, 1): ("fwd_v7<4,1>", "dgrad_v6<4>", "wgrad_v8"),
    (2, 64, 64, 2, 16, 8, 1): ("fwd_v7<3,1>", "dgrad_v6<3>", "wgrad_v8"),
    (2, 64, 64, 2, 4, 32, 1): ("fwd_v7<5,1>", "dgrad_v6<4>", "wgrad_v8"),
    # stride-2 parity classes, 8x16 dy plane
    (2, 64, 128, 2, 16, 32, 2): ("fwd_v6<4,2>", "dgrad_s2<4>", "wgrad_v8s"),
    # OC tile tail; B*OH*OW = 32 < one N tile
    (2, 64, 96, 2, 4, 4, 1): ("fwd_v6<2,1>", "dgrad_v6<2>", "wgrad_v6"),
    # half M tile; K = 288 is no multiple of 64, so no BK=64 kernel
    (2, 32, 32, 2, 4, 4, 1): ("fwd_v6<2,1>", "dgrad_v6<2>", "wgrad_v6"),
    # OW = 4, B*OH*OW = 64 (dgrad_v7<2> and wgrad_v7 under DW64)
    (2, 64, 64, 4, 4, 4, 1): ("fwd_v6<2,1>", "dgrad_v6<2>", "wgrad_v6"),
    # stride 2 at OW = 4
    (2, 64, 128, 4, 8, 8, 2): ("fwd_v6<2,2>", "dgrad_s2<2>", "wgrad_v6"),
    # stride 2 at OW = 8: the <3,2> forward kernels and dgrad_s2<3>
    (2, 64, 128, 2, 16, 16, 2): ("fwd_v6<3,2>", "dgrad_s2<3>", "wgrad_v8s"),
    # K = 288 at OW = 8 and 16: the BK=32 forward where v7 would run
    (2, 32, 32, 1, 8, 8, 1): ("fwd_v6<3,1>", "dgrad_v6<3>", "wgrad_v8"),
    (2, 32, 32, 1, 16, 16, 1): ("fwd_v6<4,1>", "dgrad_v6<4>", "wgrad_v8"),
}
V6_SHAPES = list(V6_ROUTES)

# what a variable changes in V6_ROUTES.
# OLSIM_CONV_DW64: dgrad_v7 at stride 1 when OC*9 % 64 == 0 (OC = 96 and
# 32 are not), LG_OW up to 5; wgrad_v7 when v8 / v8s do not run (OW < 8)
# and B*OH*OW % 64 == 0.  Shapes not listed keep their V6_ROUTES entry.
DW64_DGRAD_WGRAD = {
    (1, 64, 64, 1, 32, 32, 1): ("dgrad_v7<5>", "wgrad_v8"),
    (2, 64, 64, 2, 8, 16, 1): ("dgrad_v7<4>", "wgrad_v8"),
    (2, 64, 64, 2, 16, 8, 1): ("dgrad_v7<3>", "wgrad_v8"),
    (2, 64, 64, 2, 4, 32, 1): ("dgrad_v7<5>", "wgrad_v8"),
    (2, 64, 64, 4, 4, 4, 1): ("dgrad_v7<2>", "wgrad_v7"),
    (2, 64, 128, 4, 8, 8, 2): ("dgrad_s2<2>", "wgrad_v7"),
}

# shapes outside the v6 family
V5_ROUTES = {
    # OW = 2 < 4: below the v6 floor; H != W
    (2, 64, 64, 4, 8, 4, 2): ("fwd_v5<false>", "dgrad_generic", "wgrad_v5"),
    # no pow2 plane
    (2, 8, 24, 3, 6, 10, 1): ("fwd_v2", "dgrad_generic", "wgrad_generic"),
    # K = 144 is no multiple of 32 in fwd and dgrad
    (2, 16, 16, 2, 8, 16, 1): ("fwd_v2", "dgrad_generic", "wgrad_v5"),
    # odd, non-pow2, stride 2
    (1, 3, 8, 2, 7, 9, 2): ("fwd_v2", "dgrad_generic", "wgrad_generic"),
    # odd planes at stride 2 (7 -> 4): v6 and dgrad_v5 assume H = 2*OH
    (2, 64, 64, 2, 7, 7, 2): ("fwd_v5<false>", "dgrad_generic", "wgrad_v5"),
    (2, 64, 64, 2, 7, 8, 2): ("fwd_v5<false>", "dgrad_generic", "wgrad_v5"),
    # IC = 3 stem, stride 1
    (1, 3, 64, 1, 32, 32, 1): ("fwd_v2", "dgrad_v5<1>", "wgrad_v5"),
}
V5_SHAPES = list(V5_ROUTES)

# v6-family shapes run under OLSIM_CONV_V=5: fwd_v5<true> (OW >= 16) and
# <false>, dgrad_v5 at stride 1 and stride 2
FORCED_V5_ROUTES = {
    (1, 64, 64, 1, 32, 32, 1): ("fwd_v5<true>", "dgrad_v5<1>", "wgrad_v5"),
    (2, 64, 128, 2, 16, 16, 2): ("fwd_v5<false>", "dgrad_v5<2>", "wgrad_v5"),
}
FORCED_V5_SHAPES = list(FORCED_V5_ROUTES)

# OLSIM_CONV_DW8 (set, whatever its value) at OW >= 8: no wgrad_v8 / v8s
DW8_SHAPES = [
    (2, 64, 64, 2, 16, 8, 1),
    (2, 64, 128, 2, 16, 32, 2),
]

CONV3_VARS = ("OLSIM_CONV_V", "OLSIM_CONV_DW64", "OLSIM_CONV_DW8")


def _conv3_env(monkeypatch, var=None, value="1"):
    for other in CONV3_VARS:
        monkeypatch.delenv(other, raising=False)
    if var is not None:
        monkeypatch.setenv(var, value)


@pytest.mark.parametrize("shape", V6_SHAPES, ids=str)
def test_conv3x3_v6_family_bounded(shape, monkeypatch):
    _conv3_env(monkeypatch)
    _check_conv3x3(shape, True, "conv3.v6", V6_ROUTES[shape])


@pytest.mark.parametrize("shape", V5_SHAPES, ids=str)
def test_conv3x3_v5_family_bounded(shape, monkeypatch):
    _conv3_env(monkeypatch)
    _check_conv3x3(shape, False, "conv3.v5", V5_ROUTES[shape])


@pytest.mark.parametrize("var", ["OLSIM_CONV_DW64"])
@pytest.mark.parametrize("shape", V6_SHAPES, ids=str)
def test_conv3x3_env_gated_kernels_bounded(shape, var, monkeypatch):
    """dgrad_v7 / wgrad_v7 (OLSIM_CONV_DW64); the launchers read the
    environment on every call."""
    _conv3_env(monkeypatch, var)
    fwd, dgrad, wgrad = V6_ROUTES[shape]
    dgrad, wgrad = DW64_DGRAD_WGRAD.get(shape, (dgrad, wgrad))
    _check_conv3x3(shape, True, "conv3." + var.rsplit("_", 1)[1].lower(),
                   (fwd, dgrad, wgrad))


@pytest.mark.parametrize("shape", DW8_SHAPES, ids=str)
def test_conv3x3_dw8_restores_scalar_wgrad(shape, monkeypatch):
    """OLSIM_CONV_DW8=0 acts because it is set: wgrad_v6 where wgrad_v8
    (stride 1) and wgrad_v8s (stride 2) run by default."""
    _conv3_env(monkeypatch, "OLSIM_CONV_DW8", "0")
    fwd, dgrad, wgrad = V6_ROUTES[shape]
    assert wgrad in ("wgrad_v8", "wgrad_v8s")
    _check_conv3x3(shape, True, "conv3.dw8", (fwd, dgrad, "wgrad_v6"))


@pytest.mark.parametrize("shape", FORCED_V5_SHAPES, ids=str)
def test_conv3x3_forced_v5_kernels_bounded(shape, monkeypatch):
    """The pipelined v5 kernels a v6-family shape gets under
    OLSIM_CONV_V=5 (the A/B switch).  The family assertion goes through
    the dispatcher's _v6_ok, which reads the variable."""
    _conv3_env(monkeypatch, "OLSIM_CONV_V", "5")
    _check_conv3x3(shape, True, "conv3.forced_v5", FORCED_V5_ROUTES[shape],
                   forced_v5=True)


RETIRED = [("OLSIM_CONV_V8", "1"), ("OLSIM_CONV5", "direct")]


@pytest.mark.parametrize("var, value", RETIRED)
def test_retired_switches_are_ignored(var, value, monkeypatch):
    """The two settings whose kernels were retired (KERNEL_NOTES.md) change
    no route: host functions only, no kernel is launched."""
    from olearning_sim_amd.ops import load_hip_ops
    from olearning_sim_amd.ops.conv import dgrad_wt_ok
    ops = load_hip_ops(required=True)
    conv5_shapes = sorted({case[0] for case in CONV5_CASES})

    def routes():
        got = {}
        for shape in V6_SHAPES:
            C, IC, OC, B, H, W, s = shape
            got[shape] = tuple(ops.conv3x3_route(d, IC, OC, B, H, W, s)
                               for d in ("fwd", "dgrad", "wgrad")) \
                + (dgrad_wt_ok(ops, OC, IC, B, H, W, s),)
        for shape in conv5_shapes:
            C, IC, OC, B, H, W = shape
            got[shape] = tuple(ops.conv5x5_route(d, IC, OC, H, W)
                               for d in ("fwd", "dgrad", "wgrad"))
        return got

    _conv3_env(monkeypatch)
    for other, _ in RETIRED:
        monkeypatch.delenv(other, raising=False)
    unset = routes()
    for shape in V6_SHAPES:
        assert unset[shape][:3] == V6_ROUTES[shape]
    monkeypatch.setenv(var, value)
    assert routes() == unset


# ---------------------------------------------------------------------------
# conv5x5

# (shape, OLSIM_CONV5, expected fwd / dgrad / wgrad route); shapes are
# (C, IC, OC, B, H, W) with B*(H-4)*(W-4) % 32 == 0.  LDS needs in bytes:
# fwd 2*(IC*H*W + OC*IC*25), dgrad 2*(OC*(H+4)*(W+4) + OC*IC*25); the
# direct limit is 32768.  wgrad has the MFMA kernel only.
CONV5_CASES = [
    # non-square plane and the IC = OC = 16 limit
    ((2, 4, 8, 2, 12, 20), None, "direct", "direct", "mfma"),
    ((2, 16, 16, 2, 12, 12), None, "direct", "direct", "mfma"),
    # odd W: no u32 row reads.  fwd N = 288 = 2*128 + 32 and dgrad
    # N = 624 = 4*128 + 112, so both MFMA tile tails run; K = 100 -> 128
    ((2, 4, 8, 4, 12, 13), None, "mfma", "mfma", "mfma"),
    # fwd needs 39168 B; dgrad 27136 B stays direct
    ((1, 16, 8, 2, 32, 32), None, "mfma", "direct", "mfma"),
    # fwd 32376 B, just inside; dgrad 41496 B
    ((1, 12, 13, 2, 32, 32), None, "direct", "mfma", "mfma"),
    ((2, 4, 8, 2, 12, 20), "mfma", "mfma", "mfma", "mfma"),
    ((2, 16, 16, 2, 12, 12), "mfma", "mfma", "mfma", "mfma"),
    ((2, 6, 16, 8, 14, 14), "mfma", "mfma", "mfma", "mfma"),
]


def _conv5_id(case):
    return str(case[0]) if case[1] is None else f"{case[0]}:{case[1]}"


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("case", CONV5_CASES, ids=_conv5_id)
def test_conv5x5_bounded(case, relu, monkeypatch):
    """Every conv5x5 route, with the route asserted through the host
    functions the launchers branch on (the launchers read OLSIM_CONV5 on
    every call).  ReLU: signs the fp64 pre-activation cannot decide follow
    the kernel's own mask."""
    from olearning_sim_amd.ops import load_hip_ops
    from olearning_sim_amd.ops.conv import client_conv5x5, conv5x5_supported
    shape, env, r_fwd, r_dgrad, r_wgrad = case
    if env is None:
        monkeypatch.delenv("OLSIM_CONV5", raising=False)
    else:
        monkeypatch.setenv("OLSIM_CONV5", env)
    ops = load_hip_ops(required=True)
    C, IC, OC, B, H, W = shape
    assert (B * (H - 4) * (W - 4)) % 32 == 0
    assert ops.conv5x5_route("fwd", IC, OC, H, W) == r_fwd
    assert ops.conv5x5_route("dgrad", IC, OC, H, W) == r_dgrad
    assert ops.conv5x5_route("wgrad", IC, OC, H, W) == r_wgrad
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(C, IC, B, H, W, generator=g) * 0.5).to(BF)
    w = (torch.randn(C, OC, IC, 5, 5, generator=g) * 0.1).to(BF)
    b = (torch.randn(C, OC, generator=g) * 0.1).to(BF)
    dy = (torch.randn(C, OC, B, H - 4, W - 4, generator=g) * 0.1).to(BF)

    xg = x.cuda().requires_grad_(True)
    wg = w.cuda().requires_grad_(True)
    bg = b.cuda().requires_grad_(True)
    assert conv5x5_supported(xg, wg)
    y = client_conv5x5(xg, wg, bg, relu=relu)
    y.backward(dy.cuda())

    n = IC * 25 + 1
    x64, w64, b64, dy64 = upcast(x), upcast(w), upcast(b), upcast(dy)
    pre = kb.conv_math(x64, w64, 1, 0, b64)
    pre_scale = kb.conv_math(x64.abs(), w64.abs(), 1, 0, b64.abs())
    want = pre
    if relu:
        dec = kb.relu_decided(pre, pre_scale, n, BF, label="conv5")
        dy64 = dy64 * kb.relu_mask(pre, dec, y).to(dy64.dtype)
        want = pre.clamp_min(0)
    assert_bounded(y, want, pre_scale, n, BF, label="conv5.fwd")
    ref = kb.conv_ref(x64, w64, dy64, 1, 0)
    nq = B * (H - 4) * (W - 4)
    assert_bounded(xg.grad, ref["dx"], ref["dx_scale"], OC * 25, BF,
                   label="conv5.dgrad")
    assert_bounded(wg.grad, ref["dw"], ref["dw_scale"], nq, BF,
                   label="conv5.wgrad")
    assert_bounded(bg.grad, dy64.sum(dim=(2, 3, 4)),
                   dy64.abs().sum(dim=(2, 3, 4)), nq, BF, label="conv5.dbias")


# ---------------------------------------------------------------------------
# pool2x2

@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("shape", [(3, 4, 6, 10), (2, 3, 2, 8, 8)], ids=str)
def test_pool2x2_gradient_is_one_hot_per_window(shape, dtype):
    """Tie-proof and exact: y is the window maximum, and in every 2x2
    window the gradient is dy at exactly one position whose x equals the
    maximum and zero at the other three.  bf16 randn inputs contain real
    ties, so the argmax order is not assumed."""
    from olearning_sim_amd.ops.conv import max_pool2x2
    g = torch.Generator().manual_seed(21)
    x = torch.randn(*shape, generator=g).to(dtype)
    x[..., 0:2, 0:2] = 0.5                  # a window of four equal values
    H, W = shape[-2:]
    dy = torch.randn(*shape[:-2], H // 2, W // 2, generator=g).to(dtype)
    dy[dy == 0] = 1.0                       # a zero dy could not be located
    xg = x.cuda().requires_grad_(True)
    y = max_pool2x2(xg)
    y.backward(dy.cuda())

    def windows(t):                         # [..., OH, OW, 4]
        t = t.reshape(*t.shape[:-2], H // 2, 2, W // 2, 2)
        return t.transpose(-3, -2).reshape(*t.shape[:-4], H // 2, W // 2, 4)

    xw, gw = windows(x), windows(xg.grad.cpu())
    wmax = xw.max(dim=-1).values
    assert torch.equal(y.detach().cpu(), wmax)
    hit = gw != 0
    assert bool((hit.sum(-1) == 1).all()), "not exactly one routed position"
    assert torch.equal(gw.sum(-1), dy), "routed value is not dy"
    assert torch.equal(xw[hit], wmax.reshape(-1)), \
        "gradient routed to a non-maximal position"
