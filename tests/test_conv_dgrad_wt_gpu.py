"""Stride-1 conv3x3 dgrad as a forward convolution of dy_pad with the
flipped-transposed weights, against conv3x3_dgrad_p, bit for bit.

Exact equality is the derived tolerance: both kernels feed
v_mfma_f32_16x16x32_bf16 the same operands in the same K order
(k = oc*9 + r ascending in steps of 32; fwd_v7's BK = 64 is two such
sub-steps in order) into one fp32 accumulator per output element.  Each
case asserts the forward route the swapped shape reaches first, so a moved
threshold is noticed."""

import pytest
import torch

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
CONV_VARS = ("OLSIM_CONV_V", "OLSIM_CONV_DW64", "OLSIM_CONV_DW8",
             "OLSIM_CONV_NMAJOR", "OLSIM_DGRAD_WT", "OLSIM_GN_PAD")
C = 3       # client stride exercised in every case

# (IC, OC, B, H, W) of the conv whose dgrad it is -> forward route of the
# swapped shape (OC input channels, IC output channels)
CASES = {
    (64, 64, 2, 4, 4): "fwd_v6<2,1>",       # N = 32 < one 128-column tile
    (64, 64, 1, 8, 8): "fwd_v7<3,1>",
    (64, 64, 1, 16, 16): "fwd_v7<4,1>",
    (64, 64, 1, 32, 32): "fwd_v7<5,1>",
    (32, 32, 1, 8, 8): "fwd_v6<3,1>",       # OC*9 % 64 != 0
    (32, 96, 1, 16, 16): "fwd_v6<4,1>",     # 32 -> 96: K = 864, M = 32
    (96, 32, 1, 8, 8): "fwd_v6<3,1>",       # 96 -> 32: M = 96, a tail tile
    (96, 32, 3, 8, 8): "fwd_v6<3,1>",       # N = 192: full + clamped tile
}


@pytest.fixture(scope="module")
def ops():
    from olearning_sim_amd.ops import load_hip_ops
    return load_hip_ops(required=True)


@pytest.fixture(autouse=True)
def _no_conv_vars(monkeypatch):
    for var in CONV_VARS:
        monkeypatch.delenv(var, raising=False)


def _operands(IC, OC, B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(C, IC, B, H, W, generator=g) * 0.5).to(BF).cuda()
    w = (torch.randn(C, OC, IC, 3, 3, generator=g) * 0.1).to(BF).cuda()
    dy = (torch.randn(C, OC, B, H, W, generator=g) * 0.1).to(BF).cuda()
    return x, w, dy


@pytest.mark.parametrize("case", list(CASES), ids=str)
def test_fwd_on_flipped_weights_is_dgrad(ops, case):
    IC, OC, B, H, W = case
    assert ops.conv3x3_v6_ok(OC, IC, B, H, W, 1)
    assert ops.conv3x3_route("fwd", OC, IC, B, H, W, 1) == CASES[case]
    _, w, dy = _operands(*case, seed=77 + sum(case))
    dy_pad = ops.pad2d(dy, 1)
    ref = ops.conv3x3_dgrad_p(dy_pad, w, H, W, 1)
    got = ops.conv3x3_fwd_p(dy_pad, ops.conv3x3_wflip(w), 1)
    torch.cuda.synchronize()
    assert got.shape == ref.shape == (C, IC, B, H, W)
    assert torch.equal(got, ref)


# (C, IC, OC, B, H, W) -> dgrad kernel: the stride-1 shapes of
# tests/test_conv_kmajor_gpu.py (32-column segments, 4-row planes, K = 288,
# M-tile tail with N < one tile, a clamped tail tile, an XCD-padded grid)
KMAJOR_SHAPES = {
    (1, 64, 64, 1, 32, 32): "dgrad_v6<4>",
    (2, 64, 64, 2, 4, 32): "dgrad_v6<4>",
    (2, 64, 64, 2, 8, 16): "dgrad_v6<4>",
    (2, 64, 64, 2, 16, 8): "dgrad_v6<3>",
    (2, 32, 32, 1, 16, 16): "dgrad_v6<4>",
    (2, 32, 32, 1, 8, 8): "dgrad_v6<3>",
    (2, 64, 96, 2, 4, 4): "dgrad_v6<2>",
    (3, 64, 64, 3, 8, 8): "dgrad_v6<3>",
    (9, 32, 32, 1, 8, 8): "dgrad_v6<3>",
}


@pytest.mark.parametrize("shape", list(KMAJOR_SHAPES), ids=str)
def test_dgrad_v6_kmajor_still_equals_nmajor(ops, shape, monkeypatch):
    """The autograd backward no longer reaches dgrad_v6 at stride 1, so the
    dgrad half of tests/test_conv_kmajor_gpu.py (which goes through the
    backward and now compares the forward kernels on dy) is repeated here
    on conv3x3_dgrad_p itself, on the same shapes."""
    Cn, IC, OC, B, H, W = shape
    assert ops.conv3x3_route("dgrad", IC, OC, B, H, W, 1) == \
        KMAJOR_SHAPES[shape]
    g = torch.Generator().manual_seed(1234 + sum(shape))
    w = (torch.randn(Cn, OC, IC, 3, 3, generator=g) * 0.1).to(BF).cuda()
    dy = (torch.randn(Cn, OC, B, H, W, generator=g) * 0.1).to(BF).cuda()
    dy_pad = ops.pad2d(dy, 1)
    assert ops.conv3x3_staging("dgrad", IC, OC, B, H, W, 1) == "kmajor"
    km = ops.conv3x3_dgrad_p(dy_pad, w, H, W, 1)
    monkeypatch.setenv("OLSIM_CONV_NMAJOR", "1")
    assert ops.conv3x3_staging("dgrad", IC, OC, B, H, W, 1) == "nmajor"
    nm = ops.conv3x3_dgrad_p(dy_pad, w, H, W, 1)
    torch.cuda.synchronize()
    assert torch.equal(km, nm)
    # and the forward route agrees with both
    monkeypatch.delenv("OLSIM_CONV_NMAJOR")
    fw = ops.conv3x3_fwd_p(dy_pad, ops.conv3x3_wflip(w), 1)
    assert torch.equal(fw, km)


def _count_wflip(ops, monkeypatch):
    calls = []
    real = ops.conv3x3_wflip
    monkeypatch.setattr(ops, "conv3x3_wflip",
                        lambda w: (calls.append(1), real(w))[1])
    return calls


def test_dw64_keeps_the_dgrad_kernels(ops, monkeypatch):
    """OLSIM_CONV_DW64 asks for dgrad_v7 by name: the backward must then run
    conv3x3_dgrad_p, not the forward route (tests/test_conv_bounds_gpu.py
    bounds dgrad_v7 through the autograd backward)."""
    case = (64, 64, 1, 8, 8)
    IC, OC, B, H, W = case
    x, w, dy = _operands(*case, seed=13)
    calls = _count_wflip(ops, monkeypatch)
    _run_pad_fn(x, w, dy)
    assert len(calls) == 1                  # default: repack + forward route
    monkeypatch.setenv("OLSIM_CONV_DW64", "1")
    assert ops.conv3x3_route("dgrad", IC, OC, B, H, W, 1) == "dgrad_v7<3>"
    dx, _ = _run_pad_fn(x, w, dy)
    assert len(calls) == 1                  # no repack: conv3x3_dgrad_p ran
    ref = ops.conv3x3_dgrad_p(ops.pad2d(dy, 1), w, H, W, 1)
    assert torch.equal(dx, ref)


def _run_pad_fn(x, w, dy):
    from olearning_sim_amd.ops.conv import client_conv3x3
    xg = x.clone().requires_grad_(True)
    wg = w.clone().requires_grad_(True)
    client_conv3x3(xg, wg, 1).backward(dy)
    torch.cuda.synchronize()
    return xg.grad, wg.grad


@pytest.mark.parametrize("case", [(64, 64, 2, 4, 4), (32, 96, 1, 16, 16),
                                  (96, 32, 1, 8, 8)], ids=str)
def test_pad_fn_backward_switch(ops, case, monkeypatch):
    """_Conv3x3PadFn: default against OLSIM_DGRAD_WT=0."""
    x, w, dy = _operands(*case, seed=5)
    monkeypatch.setenv("OLSIM_DGRAD_WT", "0")
    dx0, dw0 = _run_pad_fn(x, w, dy)
    monkeypatch.delenv("OLSIM_DGRAD_WT")
    dx1, dw1 = _run_pad_fn(x, w, dy)
    assert torch.equal(dx1, dx0)
    assert torch.equal(dw1, dw0)


def _run_gn_fn(ops, x, w, dy, gamma, beta, res):
    from olearning_sim_amd.ops.conv import conv3x3_gn_relu
    leaves = [t.clone().requires_grad_(True) for t in (x, w, gamma, beta)]
    xg, wg, gg, bg = leaves
    # x as a padded pair, the way the model hands it over
    y, y_pad = conv3x3_gn_relu(xg, ops.pad2d(x, 1), wg, 1, C, 8, gg, bg,
                               res=res, pad_out=False)
    assert y_pad is None
    y.backward(dy)
    torch.cuda.synchronize()
    return [t.grad for t in leaves]


@pytest.mark.parametrize("case", [(64, 64, 2, 4, 4), (64, 64, 2, 8, 8)],
                         ids=str)
def test_gn_pad_fn_backward_switch(ops, case, monkeypatch):
    """_Conv3x3GnPadFn: default against OLSIM_DGRAD_WT=0; dx, dw, dgamma,
    dbeta.  The GN backward's dgamma/dbeta atomics have been bit-stable at
    these sizes (tests/test_gn_pad_gpu.py), so all four are compared
    exactly."""
    from olearning_sim_amd.ops.fused import gn_pad_shape_ok
    IC, OC, B, H, W = case
    assert gn_pad_shape_ok(OC, 8, H, W)      # the fused node is what runs
    x, w, dy = _operands(*case, seed=9)
    g = torch.Generator().manual_seed(11)
    gamma = (1 + 0.1 * torch.randn(C, OC, generator=g)).to(BF).cuda()
    beta = (0.1 * torch.randn(C, OC, generator=g)).to(BF).cuda()
    res = (torch.randn(C, OC, B, H, W, generator=g) * 0.5).to(BF).cuda()
    monkeypatch.setenv("OLSIM_DGRAD_WT", "0")
    off = _run_gn_fn(ops, x, w, dy, gamma, beta, res)
    monkeypatch.delenv("OLSIM_DGRAD_WT")
    on = _run_gn_fn(ops, x, w, dy, gamma, beta, res)
    for name, a, b in zip(("dx", "dw", "dgamma", "dbeta"), on, off):
        assert torch.equal(a, b), name
