"""k-major B staging of the stride-1 conv3x3 fwd / dgrad kernels against
the [n][k] staging it replaces (OLSIM_CONV_NMAJOR), bit for bit.

Exact equality is the derived tolerance: the staging changes how the B
tile lies in LDS and how it is read back, not which 8 k enter which MFMA
or in which order, so every accumulator sees the same operands in the
same sequence.  Each case asserts ops.conv3x3_staging before each run,
so it cannot pass by comparing the [n][k] kernels with themselves."""

import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
DIRS = ("fwd", "dgrad")
CONV_VARS = ("OLSIM_CONV_V", "OLSIM_CONV_DW64", "OLSIM_CONV_DW8",
             "OLSIM_CONV_NMAJOR")

# (C, IC, OC, B, H, W, stride) -> the (fwd, dgrad) kernels it reaches
SHAPES = {
    # 32-column segments of fwd_v7<5,1>
    (1, 64, 64, 1, 32, 32, 1): ("fwd_v7<5,1>", "dgrad_v6<4>"),
    # the same at a 4-row plane
    (2, 64, 64, 2, 4, 32, 1): ("fwd_v7<5,1>", "dgrad_v6<4>"),
    (2, 64, 64, 2, 8, 16, 1): ("fwd_v7<4,1>", "dgrad_v6<4>"),
    (2, 64, 64, 2, 16, 8, 1): ("fwd_v7<3,1>", "dgrad_v6<3>"),
    # K = 288: the BK=32 forward
    (2, 32, 32, 1, 16, 16, 1): ("fwd_v6<4,1>", "dgrad_v6<4>"),
    (2, 32, 32, 1, 8, 8, 1): ("fwd_v6<3,1>", "dgrad_v6<3>"),
    # M-tile tail, N = 32 < one tile
    (2, 64, 96, 2, 4, 4, 1): ("fwd_v6<2,1>", "dgrad_v6<2>"),
    # N = 192: a full tile and a clamped tail tile
    (3, 64, 64, 3, 8, 8, 1): ("fwd_v7<3,1>", "dgrad_v6<3>"),
    # XCD remap tail: the grid is padded to 16 clients
    (9, 32, 32, 1, 8, 8, 1): ("fwd_v6<3,1>", "dgrad_v6<3>"),
}

# (direction, shape) that conv3_route.h keeps on the [n][k] staging because
# the k-major kernel measured no faster there: asserted "nmajor", nothing
# to compare.  fwd_v7<3,1> is the one such kernel (1.3 % slower k-major,
# profiles/conv_kmajor_r06.md); LG_OW = 3 stays covered by fwd_v6<3,1>
# and dgrad_v6<3>.
NMAJOR_GATED: set = {
    ("fwd", (2, 64, 64, 2, 16, 8, 1)),
    ("fwd", (3, 64, 64, 3, 8, 8, 1)),
}


@pytest.fixture(scope="module")
def ops():
    from olearning_sim_amd.ops import load_hip_ops
    return load_hip_ops(required=True)


@pytest.fixture(autouse=True)
def _no_conv_vars(monkeypatch):
    for var in CONV_VARS:
        monkeypatch.delenv(var, raising=False)


def _staging(ops, shape):
    C, IC, OC, B, H, W, s = shape
    return tuple(ops.conv3x3_staging(d, IC, OC, B, H, W, s) for d in DIRS)


def _routes(ops, shape, dirs=DIRS):
    C, IC, OC, B, H, W, s = shape
    return tuple(ops.conv3x3_route(d, IC, OC, B, H, W, s) for d in dirs)


def _run(x, w, dy, s):
    from olearning_sim_amd.ops.conv import client_conv3x3
    xg = x.clone().requires_grad_(True)
    wg = w.clone().requires_grad_(True)
    y = client_conv3x3(xg, wg, s)
    y.backward(dy)
    torch.cuda.synchronize()
    return y.detach(), xg.grad


@pytest.mark.parametrize("shape", list(SHAPES), ids=str)
def test_kmajor_bit_identical_to_nmajor(ops, shape, monkeypatch):
    C, IC, OC, B, H, W, s = shape
    assert _routes(ops, shape) == SHAPES[shape]
    g = torch.Generator().manual_seed(1234 + sum(shape))
    x = (torch.randn(C, IC, B, H, W, generator=g) * 0.5).to(BF).cuda()
    w = (torch.randn(C, OC, IC, 3, 3, generator=g) * 0.1).to(BF).cuda()
    dy = (torch.randn(C, OC, B, H, W, generator=g) * 0.1).to(BF).cuda()

    expect = tuple("nmajor" if (d, shape) in NMAJOR_GATED else "kmajor"
                   for d in DIRS)
    assert _staging(ops, shape) == expect
    y_new, dx_new = _run(x, w, dy, s)

    monkeypatch.setenv("OLSIM_CONV_NMAJOR", "1")
    assert _staging(ops, shape) == ("nmajor", "nmajor")
    y_old, dx_old = _run(x, w, dy, s)

    assert y_old.abs().max() > 0 and dx_old.abs().max() > 0
    if expect[0] == "kmajor":
        assert torch.equal(y_new, y_old), \
            f"fwd: {(y_new != y_old).sum().item()} of {y_old.numel()} differ"
    if expect[1] == "kmajor":
        assert torch.equal(dx_new, dx_old), \
            f"dgrad: {(dx_new != dx_old).sum().item()} of {dx_old.numel()} differ"


def test_gating_leaves_every_lg_ow_compared():
    # only gated shapes skip the comparison, never a whole LG_OW: each
    # direction keeps a compared k-major case at every LG_OW it is built for
    def lg(route):
        return int(route.split("<")[1][0])
    for di, d in enumerate(DIRS):
        every = {lg(r[di]) for r in SHAPES.values()}
        live = {lg(SHAPES[sh][di]) for sh in SHAPES
                if (d, sh) not in NMAJOR_GATED}
        assert live == every, f"{d}: LG_OW {every - live} is never compared"
    assert all(sh in SHAPES for _, sh in NMAJOR_GATED)


@pytest.mark.parametrize("shape", list(SHAPES), ids=str)
def test_routes_do_not_depend_on_staging(ops, shape, monkeypatch):
    dirs = ("fwd", "dgrad", "wgrad")
    before = _routes(ops, shape, dirs)
    assert before[:2] == SHAPES[shape]
    monkeypatch.setenv("OLSIM_CONV_NMAJOR", "1")
    assert _routes(ops, shape, dirs) == before


def test_staging_of_unconverted_kernels(ops, monkeypatch):
    # wgrad, stride 2 and the v5 family have no k-major form
    assert ops.conv3x3_staging("wgrad", 64, 64, 1, 32, 32, 1) == "nmajor"
    for d in DIRS:
        assert ops.conv3x3_staging(d, 64, 128, 2, 16, 32, 2) == "nmajor"
        assert ops.conv3x3_staging(d, 8, 24, 3, 6, 10, 1) == "nmajor"
    # the env-gated record keeps the staging it was measured with
    monkeypatch.setenv("OLSIM_CONV_DW64", "1")
    assert ops.conv3x3_staging("dgrad", 64, 64, 1, 32, 32, 1) == "nmajor"
    monkeypatch.delenv("OLSIM_CONV_DW64")
    monkeypatch.setenv("OLSIM_CONV_V", "5")
    assert ops.conv3x3_staging("fwd", 64, 64, 1, 32, 32, 1) == "nmajor"
