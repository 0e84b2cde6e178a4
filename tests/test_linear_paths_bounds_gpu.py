"""The GPU-only linear paths against fp64 with the derived bounds of
tests/kernel_bounds.py: the per-client linear's hand-written backward
(models/base.py _BLinearFn, both transpose kernels), the 1x1 conv and
its three stride-2 routes, the sliced tied-head cross-entropy, and the
MLP / LSTM / BERT gradients in fp32 against the same model in fp64."""

import pytest
import torch

import kernel_bounds as kb
from kernel_bounds import assert_bounded, upcast

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module", autouse=True)
def _require_ext():
    from olearning_sim_amd.ops import load_hip_ops
    load_hip_ops(required=True)


class _CountingOps:
    """The extension namespace with transpose2d calls recorded as (M, N)."""

    def __init__(self, ops):
        self._ops = ops
        self.transposes = []

    def __getattr__(self, name):
        return getattr(self._ops, name)

    def transpose2d(self, x):
        self.transposes.append((x.shape[1], x.shape[2]))
        return self._ops.transpose2d(x)

    def thin(self):
        return [s for s in self.transposes if s[0] <= 32 and s[0] % 8 == 0]

    def tiled(self):
        return [s for s in self.transposes
                if not (s[0] <= 32 and s[0] % 8 == 0)]


@pytest.fixture
def counting_ops(monkeypatch):
    from olearning_sim_amd.ops import fused
    proxy = _CountingOps(fused.load_hip_ops(required=True))
    monkeypatch.setattr(fused, "_HIP_OPS", proxy)
    return proxy


# ---------------------------------------------------------------------------
# per-client linear

# (C, rows, in, out) -> kernels fast_transpose(x) / fast_transpose(w) take
BLINEAR_SHAPES = [
    ((3, 8, 40, 24), "thin", "tiled"),
    ((2, 32, 400, 120), "thin", "tiled"),   # LeNet fc1: thin with chunk tail
    ((2, 16, 84, 10), "thin", "tiled"),
    ((2, 12, 8, 64), "tiled", "thin"),      # x tiled edge, w thin at M = 8
    ((1, 40, 64, 64), "tiled", "tiled"),    # w exactly one full tile
]


def _run_blinear(x, w, b, dy):
    from olearning_sim_amd.models.base import blinear
    xg = x.cuda().requires_grad_(True)
    wg = w.cuda().requires_grad_(True)
    bg = None if b is None else b.cuda().requires_grad_(True)
    y = blinear(xg, wg, bg)
    y.backward(dy)
    got = {"y": y, "dx": xg.grad, "dw": wg.grad}
    if bg is not None:
        got["db"] = bg.grad
    return got


@pytest.mark.parametrize("has_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("dtype", [BF, F32], ids=str)
@pytest.mark.parametrize("case", BLINEAR_SHAPES, ids=lambda c: str(c[0]))
def test_blinear_bounded(case, dtype, has_bias, counting_ops):
    """y, dx (through a materialised w^T), dw (through a materialised
    x^T) and db of _BLinearFn; the transposes must have taken the kernels
    the shape is here for."""
    (C, rows, fin, fout), x_route, w_route = case
    g = torch.Generator().manual_seed(rows * 1000 + fin)
    x = torch.randn(C, rows, fin, generator=g).to(dtype)
    w = (torch.randn(C, fin, fout, generator=g) * 0.2).to(dtype)
    b = torch.randn(C, fout, generator=g).to(dtype) if has_bias else None
    dy = (torch.randn(C, rows, fout, generator=g) * 0.1).to(dtype)
    got = _run_blinear(x, w, b, dy.cuda())
    assert sorted(counting_ops.transposes) == sorted([(rows, fin),
                                                      (fin, fout)])
    assert len(counting_ops.thin()) == [x_route, w_route].count("thin")
    ref = kb.linear_math(upcast(x), upcast(w),
                         None if b is None else upcast(b), upcast(dy))
    kb.assert_linear_bounded(got, ref, dtype, has_bias)


def test_blinear_noncontiguous_upstream_gradient_bounded(counting_ops):
    """dy arrives as a transposed view; the backward must make it
    contiguous before the GEMMs and the bias sum."""
    C, rows, fin, fout = 3, 8, 40, 24
    g = torch.Generator().manual_seed(5)
    x = torch.randn(C, rows, fin, generator=g).to(BF)
    w = (torch.randn(C, fin, fout, generator=g) * 0.2).to(BF)
    b = torch.randn(C, fout, generator=g).to(BF)
    dy_t = (torch.randn(C, fout, rows, generator=g) * 0.1).to(BF).cuda()
    dy = dy_t.transpose(1, 2)
    assert not dy.is_contiguous()
    got = _run_blinear(x, w, b, dy)
    assert len(counting_ops.transposes) == 2
    ref = kb.linear_math(upcast(x), upcast(w), upcast(b), upcast(dy))
    kb.assert_linear_bounded(got, ref, BF, True, label="blinear.strided_dy")


# ---------------------------------------------------------------------------
# 1x1 conv

def _conv1x1(x, w, dy, stride, padded):
    from olearning_sim_amd.ops import load_hip_ops
    from olearning_sim_amd.ops.conv import client_conv1x1
    xg = x.cuda().requires_grad_(True)
    wg = w.cuda().requires_grad_(True)
    x_pad = load_hip_ops(required=True).pad2d(xg.detach(), 1) \
        if padded else None
    y = client_conv1x1(xg, wg, stride, x_pad=x_pad)
    y.backward(dy.cuda())
    return y.detach(), xg.grad, wg.grad


@pytest.mark.parametrize("shape,stride,padded", [
    ((2, 64, 128, 2, 8, 8), 1, False),
    ((2, 64, 128, 2, 8, 8), 2, False),     # subsample kernel
    ((2, 64, 128, 2, 8, 8), 2, True),      # padded pair: reads x_pad
    ((2, 16, 32, 2, 6, 6), 2, False),      # W % 4 != 0: slicing fallback
], ids=str)
def test_conv1x1_bounded(shape, stride, padded):
    """fwd, dx and dw of the 1x1 conv (one bmm over clients) and of the
    stride-2 subsample in front of it; reduction lengths IC, OC and
    B*OH*OW.  The padded-pair route must equal the dense one bit for bit:
    both read the same pixels."""
    C, IC, OC, B, H, W = shape
    OH, OW = (H + stride - 1) // stride, (W + stride - 1) // stride
    g = torch.Generator().manual_seed(IC + stride)
    x = (torch.randn(C, IC, B, H, W, generator=g) * 0.5).to(BF)
    w = (torch.randn(C, OC, IC, generator=g) * 0.1).to(BF)
    dy = (torch.randn(C, OC, B, OH, OW, generator=g) * 0.1).to(BF)
    y, dx, dw = _conv1x1(x, w, dy, stride, padded)
    assert y.shape == (C, OC, B, OH, OW)
    if padded:
        for a, b_ in zip((y, dx, dw), _conv1x1(x, w, dy, stride, False)):
            assert torch.equal(a, b_)
    ref = kb.conv_ref(upcast(x), upcast(w).view(C, OC, IC, 1, 1), upcast(dy),
                      stride, 0)
    assert_bounded(y, ref["y"], ref["y_scale"], IC, BF, label="conv1.fwd")
    assert_bounded(dx, ref["dx"], ref["dx_scale"], OC, BF, label="conv1.dx")
    assert_bounded(dw, ref["dw"].view(C, OC, IC),
                   ref["dw_scale"].view(C, OC, IC), B * OH * OW, BF,
                   label="conv1.dw")


# ---------------------------------------------------------------------------
# tied head + cross-entropy

@pytest.mark.parametrize("dtype", [F32, BF], ids=str)
def test_tied_head_ce_bounded(dtype, monkeypatch, counting_ops):
    """_TiedHeadCE at SLICE_V = 16 over V = 40: two full slices and an
    8-wide tail, with labels on both sides of every slice boundary.  fp32
    is the sharp check of the sliced algorithm; bf16 checks the
    production dtype's conversions.  Bound: kb.assert_tied_head_bounded."""
    from olearning_sim_amd.models.bert import _TiedHeadCE, tied_head_ce
    monkeypatch.setattr(_TiedHeadCE, "SLICE_V", 16)
    C, N, H, V = 2, 8, 16, 40
    g = torch.Generator().manual_seed(23)
    hs = torch.randn(C, N, H, generator=g).to(dtype)
    tok = (torch.randn(C, V, H, generator=g) * 0.5).to(dtype)
    bias = (torch.randn(C, V, generator=g) * 0.5).to(dtype)
    labels = torch.tensor([[0, 15, 16, 31, 32, 39, 7, 20],
                           [39, 32, 31, 16, 15, 0, 33, 8]])
    leaves = [t.cuda().requires_grad_(True) for t in (hs, tok, bias)]
    loss = tied_head_ce(*leaves, labels.cuda())
    loss.backward()
    assert counting_ops.transposes == [(V, H)]
    got = {"loss": loss.detach(), "dhs": leaves[0].grad,
           "dtok": leaves[1].grad, "dbias": leaves[2].grad}
    assert got["loss"].dtype == F32
    ref = kb.tied_head_math(upcast(hs), upcast(tok), upcast(bias), labels, 16)
    kb.assert_tied_head_bounded(got, ref, upcast(hs), upcast(tok), dtype, 16)


# ---------------------------------------------------------------------------
# model gradients, fp32 on the device against fp64

def _gpu_model_run(name):
    case = kb.model_case(name)
    params = {k: v.cuda() for k, v in case["params"].items()}
    loss, grads = kb.model_loss_and_grads(case["model"], params,
                                          case["x"].cuda(), case["y"].cuda())
    return kb.assert_model_bounded(name, loss, grads)


def test_mlp_gradients_fp32_match_fp64(counting_ops):
    _gpu_model_run("mlp")
    # x [3, 8, 40] and h [3, 8, 24] thin, fc2.w [3, 24, 10] thin,
    # fc1.w [3, 40, 24] tiled (fc1 has no dx: its input is data)
    assert sorted(counting_ops.thin()) == [(8, 24), (8, 40), (24, 10)]
    assert counting_ops.tiled() == []


def test_lstm_gradients_fp32_match_fp64(counting_ops):
    _gpu_model_run("lstm")
    # per layer: the input projection (x^T, w_ih^T) and L = 4 recurrence
    # steps (h^T, w_hh^T; the first step's h is a constant zero, so it has
    # no dx and no w_hh^T): 2 + 7; then the head's two.  Every one is
    # thin: rows 8 or 32, embed 8, hidden 16.
    assert counting_ops.tiled() == []
    assert len(counting_ops.thin()) == 2 * (2 + 7) + 2
    assert (8, 64) in counting_ops.thin()          # l0.w_ih at embed = 8


def test_bert_gradients_fp32_match_fp64(counting_ops, monkeypatch):
    from olearning_sim_amd.models.bert import _TiedHeadCE
    from olearning_sim_amd.ops import fused
    monkeypatch.setattr(_TiedHeadCE, "SLICE_V", 16)
    seen = []
    real_layernorm = fused.layernorm

    def layernorm(*a, **kw):
        out = real_layernorm(*a, **kw)
        seen.append(out is not None)
        return out

    monkeypatch.setattr(fused, "layernorm", layernorm)
    _gpu_model_run("bert")
    assert seen == [True] * 5, "a LayerNorm fell back to the composed path"
    assert (40, 32) in counting_ops.tiled()        # tied head tok^T
    assert counting_ops.thin()                     # rows = B*L = 32
