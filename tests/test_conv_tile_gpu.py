"""128x64 block tile of the conv3x3 forward kernels against the 64x128
tile it replaces (OLSIM_CONV_BM64), bit for bit.

Exact equality is the derived tolerance: the tile changes which wave owns
which rows and how many columns a block stages, not which 8 k enter which
MFMA or in which order, so every accumulator sees the same operands in the
same sequence.  Each case asserts ops.conv3x3_tile before each run, so it
cannot pass by comparing the 64x128 kernels with themselves."""

import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
CONV_VARS = ("OLSIM_CONV_V", "OLSIM_CONV_DW64", "OLSIM_CONV_DW8",
             "OLSIM_CONV_NMAJOR", "OLSIM_CONV_BM64", "OLSIM_DGRAD_WT")
TALL, WIDE = "128x64", "64x128"

# (C, IC, OC, B, H, W, stride) -> the forward kernel it reaches
SHAPES = {
    # N = 32 < one tile
    (2, 64, 128, 2, 4, 4, 1): "fwd_v6<2,1>",
    # M tail, rows 96..127 masked
    (2, 64, 96, 2, 4, 4, 1): "fwd_v6<2,1>",
    # N = 64, exactly one tile
    (2, 32, 128, 1, 8, 8, 1): "fwd_v6<3,1>",
    # two m-tiles
    (1, 32, 256, 1, 8, 8, 1): "fwd_v6<3,1>",
    # XCD remap tail: the grid is padded to 16 clients
    (9, 32, 128, 1, 8, 8, 1): "fwd_v6<3,1>",
    (2, 32, 128, 1, 16, 16, 1): "fwd_v6<4,1>",
    (2, 64, 128, 2, 16, 8, 1): "fwd_v7<3,1>",
    # N = 96: a full tile and a clamped tail tile
    (3, 64, 128, 3, 4, 8, 1): "fwd_v7<3,1>",
    (2, 64, 128, 2, 8, 16, 1): "fwd_v7<4,1>",
    (1, 64, 128, 1, 32, 32, 1): "fwd_v7<5,1>",
    (2, 64, 128, 2, 4, 32, 1): "fwd_v7<5,1>",
    # stride 2: dx comes from dgrad_s2, which has the one tile; compare y
    (2, 64, 128, 2, 8, 8, 2): "fwd_v6<2,2>",
    (2, 64, 128, 2, 16, 16, 2): "fwd_v6<3,2>",
    (1, 64, 128, 1, 32, 32, 2): "fwd_v6<4,2>",
}

# forward kernel -> why conv3_route.h keeps it on the 64x128 tile although
# the shape qualifies (measured no faster on the tall tile): asserted
# "64x128", nothing to compare
GATED: dict = {}


@pytest.fixture(scope="module")
def ops():
    from olearning_sim_amd.ops import load_hip_ops
    return load_hip_ops(required=True)


@pytest.fixture(autouse=True)
def _no_conv_vars(monkeypatch):
    for var in CONV_VARS:
        monkeypatch.delenv(var, raising=False)


def _tile(ops, shape):
    C, IC, OC, B, H, W, s = shape
    return ops.conv3x3_tile("fwd", IC, OC, B, H, W, s)


def _routes(ops, shape):
    C, IC, OC, B, H, W, s = shape
    return tuple(ops.conv3x3_route(d, IC, OC, B, H, W, s)
                 for d in ("fwd", "dgrad", "wgrad"))


def _operands(shape):
    C, IC, OC, B, H, W, s = shape
    g = torch.Generator().manual_seed(4321 + sum(shape))
    x = (torch.randn(C, IC, B, H, W, generator=g) * 0.5).to(BF).cuda()
    w = (torch.randn(C, OC, IC, 3, 3, generator=g) * 0.1).to(BF).cuda()
    dy = (torch.randn(C, OC, B, -(-H // s), -(-W // s), generator=g)
          * 0.1).to(BF).cuda()
    return x, w, dy


def _run(x, w, dy, s):
    from olearning_sim_amd.ops.conv import client_conv3x3
    xg = x.clone().requires_grad_(True)
    wg = w.clone().requires_grad_(True)
    y = client_conv3x3(xg, wg, s)
    y.backward(dy)
    torch.cuda.synchronize()
    return y.detach(), xg.grad


@pytest.mark.parametrize("shape", list(SHAPES), ids=str)
def test_tall_tile_bit_identical_to_wide(ops, shape, monkeypatch):
    s = shape[-1]
    routes = _routes(ops, shape)
    assert routes[0] == SHAPES[shape]
    x, w, dy = _operands(shape)

    expect = WIDE if SHAPES[shape] in GATED else TALL
    assert _tile(ops, shape) == expect
    y_new, dx_new = _run(x, w, dy, s)

    # the [n][k] staging of the same tile
    monkeypatch.setenv("OLSIM_CONV_NMAJOR", "1")
    assert _tile(ops, shape) == expect
    y_nm, _ = _run(x, w, dy, s)
    monkeypatch.delenv("OLSIM_CONV_NMAJOR")

    monkeypatch.setenv("OLSIM_CONV_BM64", "1")
    assert _tile(ops, shape) == WIDE
    assert _routes(ops, shape) == routes
    y_old, dx_old = _run(x, w, dy, s)

    assert y_old.abs().max() > 0 and dx_old.abs().max() > 0
    assert torch.equal(y_new, y_old), \
        f"fwd: {(y_new != y_old).sum().item()} of {y_old.numel()} differ"
    assert torch.equal(y_nm, y_old), \
        f"fwd [n][k]: {(y_nm != y_old).sum().item()} of {y_old.numel()} differ"
    if s == 1:
        assert torch.equal(dx_new, dx_old), \
            f"dgrad: {(dx_new != dx_old).sum().item()} of {dx_old.numel()} differ"


def test_flipped_weight_dgrad_takes_the_swapped_forwards_tile(ops, monkeypatch):
    shape = (2, 128, 64, 2, 8, 8, 1)
    C, IC, OC, B, H, W, s = shape
    x, w, dy = _operands(shape)
    # the forward has 64 output channels; its dgrad is the forward of
    # (OC input channels, IC = 128 output channels)
    assert _tile(ops, shape) == WIDE
    assert ops.conv3x3_route("fwd", OC, IC, B, H, W, 1) == "fwd_v7<3,1>"
    expect = WIDE if "fwd_v7<3,1>" in GATED else TALL
    assert ops.conv3x3_tile("fwd", OC, IC, B, H, W, 1) == expect
    y_new, dx_new = _run(x, w, dy, s)
    monkeypatch.setenv("OLSIM_CONV_BM64", "1")
    assert _tile(ops, shape) == WIDE
    assert ops.conv3x3_tile("fwd", OC, IC, B, H, W, 1) == WIDE
    y_old, dx_old = _run(x, w, dy, s)
    assert dx_old.abs().max() > 0
    assert torch.equal(dx_new, dx_old)
    assert torch.equal(y_new, y_old)


def test_shapes_that_keep_the_wide_tile(ops, monkeypatch):
    # the taller tile would add padded rows
    assert ops.conv3x3_tile("fwd", 64, 64, 1, 32, 32, 1) == WIDE
    assert ops.conv3x3_tile("fwd", 64, 192, 1, 8, 8, 1) == WIDE
    # dgrad and wgrad kernels have the one tile
    for shape in SHAPES:
        C, IC, OC, B, H, W, s = shape
        for d in ("dgrad", "wgrad"):
            assert ops.conv3x3_tile(d, IC, OC, B, H, W, s) == WIDE
    # the v5 family keeps its own
    probe = (2, 64, 128, 2, 8, 16, 1)
    if SHAPES[probe] not in GATED:
        assert _tile(ops, probe) == TALL
    monkeypatch.setenv("OLSIM_CONV_V", "5")
    assert _tile(ops, probe) == WIDE


def test_every_tall_instantiation_is_compared():
    # every forward kernel built for the 128x64 tile keeps a compared case;
    # a kernel gated back is listed with its reason, and its shapes stay in
    # SHAPES (asserted "64x128" above)
    every = {"fwd_v6<2,1>", "fwd_v6<3,1>", "fwd_v6<4,1>", "fwd_v6<2,2>",
             "fwd_v6<3,2>", "fwd_v6<4,2>", "fwd_v7<3,1>", "fwd_v7<4,1>",
             "fwd_v7<5,1>"}
    assert set(SHAPES.values()) == every
    assert set(GATED) <= every
    assert all(reason for reason in GATED.values())
    live = {r for r in SHAPES.values() if r not in GATED}
    assert live == every - set(GATED)
