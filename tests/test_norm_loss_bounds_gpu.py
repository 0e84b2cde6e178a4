"""Cross-entropy, LayerNorm, dense GroupNorm, fused SGD/FedProx and
delta-accumulation kernels against fp64 references, with the derived
element-wise bounds of tests/kernel_bounds.py (no fitted tolerances).

References are computed in fp64 from upcast copies of the exact tensors
the kernels receive; scalars are taken at the fp32 value the launcher
passes."""

import pytest
import torch

import kernel_bounds as kb
from kernel_bounds import assert_bounded, upcast

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
DTYPES = [pytest.param(F32, id="f32"), pytest.param(BF, id="bf16")]


@pytest.fixture(scope="module", autouse=True)
def _require_ext():
    from olearning_sim_amd.ops import load_hip_ops
    load_hip_ops(required=True)


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


# ---------------------------------------------------------------------------
# cross-entropy

def _check_ce(logits, labels):
    from olearning_sim_amd.ops import fused
    dtype = logits.dtype
    N, K = logits.shape
    lg = logits.cuda().requires_grad_(True)
    loss = fused.cross_entropy_fwd_bwd(lg, labels.cuda())
    (3 * loss).backward()                    # upstream gradient applied
    ref = kb.ce_math(upcast(logits), labels, upstream=3.0)
    assert loss.dtype == F32
    assert_bounded(loss, ref["loss"], ref["loss_scale"], K + N, F32,
                   intrinsic=True, label="ce.loss")
    # two roundings to the logits dtype: the kernel stores dlogits, the
    # autograd backward multiplies the stored tensor by the upstream 3
    assert_bounded(lg.grad, ref["grad"], ref["grad_scale"], K, dtype,
                   intrinsic=True, label="ce.grad", roundings=2)


def _ce_inputs(N, K, dtype, seed=1, amp=3.0):
    g = torch.Generator().manual_seed(seed)
    logits = (torch.randn(N, K, generator=g) * amp).to(dtype)
    labels = torch.randint(0, K, (N,), generator=g)
    labels[0], labels[1], labels[N - 1] = 0, K - 1, K - 1
    return logits, labels


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [8, 256])
@pytest.mark.parametrize("K", [2, 10, 511, 512, 513, 30522])
def test_cross_entropy_bounded(dtype, N, K):
    """K = 512 is where the launcher switches from one wave to a full
    workgroup per row; labels 0 and K-1 are forced into some rows."""
    _check_ce(*_ce_inputs(N, K, dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_cross_entropy_grid_stride_rows(dtype):
    """N > 16384 rows: the grid is capped and rows are grid-strided."""
    _check_ce(*_ce_inputs(16384 + 5, 10, dtype, seed=2))


def test_cross_entropy_large_logits_max_subtraction():
    """fp32 logits spanning +-80: exp() without the max subtraction
    overflows at 88.7; far tails legitimately flush to zero."""
    logits, labels = _ce_inputs(64, 513, F32, seed=3)
    logits = logits * (80.0 / float(logits.abs().max()))
    assert float(logits.max()) > 79 or float(logits.min()) < -79
    _check_ce(logits, labels)


# ---------------------------------------------------------------------------
# LayerNorm

LN_SHAPES = [(3, 8, 768), (5, 4, 128), (2, 4, 8), (2, 4, 520), (1, 4, 1536)]


def _check_layernorm(x0, dtype, seed):
    from olearning_sim_amd.ops.fused import layernorm
    g = torch.Generator().manual_seed(seed)
    C, N, H = x0.shape
    x = x0.to(dtype)
    gamma = (torch.randn(C, H, generator=g) * 0.5 + 1.0).to(dtype)
    beta = (torch.randn(C, H, generator=g) * 0.2).to(dtype)
    dy = (torch.randn(C, N, H, generator=g) * 0.1).to(dtype)

    xg = x.cuda().requires_grad_(True)
    gg = gamma.cuda().requires_grad_(True)
    bg = beta.cuda().requires_grad_(True)
    y = layernorm(xg, gg, bg)
    assert y is not None, "fused LayerNorm kernel not taken"
    y.backward(dy.cuda())

    r = kb.norm_math(upcast(x), upcast(gamma).unsqueeze(1),
                     upcast(beta).unsqueeze(1), (-1,), _f32(1e-5),
                     dy=upcast(dy))
    assert_bounded(y, r["pre"], r["pre_scale"], H, dtype, intrinsic=True,
                   label="ln.y")
    assert_bounded(xg.grad, r["dx"], r["dx_scale"], H, dtype, intrinsic=True,
                   label="ln.dx")
    # dgamma sums N terms g*xhat, each xhat carrying its own H-term error
    assert_bounded(gg.grad, r["gx"].sum(1), r["gx_scale"].sum(1), N + H,
                   dtype, intrinsic=True, label="ln.dgamma")
    assert_bounded(bg.grad, r["g"].sum(1), r["g"].abs().sum(1), N, dtype,
                   label="ln.dbeta")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", LN_SHAPES, ids=str)
def test_layernorm_bounded(shape, dtype):
    g = torch.Generator().manual_seed(9)
    _check_layernorm(torch.randn(*shape, generator=g) * 2 + 0.3, dtype, 10)


@pytest.mark.parametrize("dtype", DTYPES)
def test_layernorm_shifted_mean_bounded(dtype):
    """x = 8 + 0.5*randn: the kernel's E[x^2] - mean^2 cancels 8 bits."""
    g = torch.Generator().manual_seed(11)
    _check_layernorm(8 + 0.5 * torch.randn(3, 8, 768, generator=g), dtype, 12)


# ---------------------------------------------------------------------------
# dense GroupNorm (both layouts, LDS-staged and streaming kernels)

G = 8
# bf16 reaches k_gn_fwd_lds/k_gn_bwd_lds when HW % 8 == 0 and the group
# plane fits 64 KB; HW = 4 and HW = 36 take the scalar streaming kernels,
# (1,256,1,32,32) stages the forward in LDS but streams the backward,
# fp32 always streams (vector path when HW % 8 == 0).
# HW % 8 == 0 with HW/8 not a power of two (28x28: 98 vectors per plane,
# 4x6: 3) is where the backward's per-channel lane groups must not
# straddle a channel: dgamma/dbeta were summed across channels there.
GN_SHAPES = [(2, 64, 2, 8, 8), (1, 16, 1, 4, 8), (3, 16, 2, 2, 2),
             (2, 16, 1, 6, 6), (1, 256, 1, 32, 32), (1, 1024, 1, 2, 4),
             (1, 16, 1, 28, 28), (2, 16, 2, 4, 6),
             (4, 5, 64, 8, 8), (2, 3, 16, 4, 6)]
# the last two entries are 4-D, given as (B, C, ch, H, W)
GN_LAYOUT = [1, 1, 1, 1, 1, 1, 1, 1, 0, 0]


def _check_groupnorm(shape, layout, relu, res, dtype, shift=False,
                     pad=False):
    from olearning_sim_amd.ops.fused import (gn_pad_eligible, groupnorm_act,
                                             groupnorm_relu_pad, load_hip_ops)
    ops = load_hip_ops(required=True)
    g = torch.Generator().manual_seed(0)
    if layout == 1:
        C, ch, B, H, W = shape
        xshape = (C, ch, B, H, W)
    else:
        B, C, ch, H, W = shape
        xshape = (B, C * ch, H, W)
    cg, HW = ch // G, H * W
    n = cg * HW
    x = torch.randn(*xshape, generator=g)
    if shift:
        x = 8 + 0.5 * x
    x = x.to(dtype)
    gamma = (1 + 0.1 * torch.randn(C, ch, generator=g)).to(dtype)
    beta = (0.1 * torch.randn(C, ch, generator=g)).to(dtype)
    resid = torch.randn(*xshape, generator=g).to(dtype) if res else None
    dy = torch.randn(*xshape, generator=g).to(dtype)

    xg = x.cuda().requires_grad_(True)
    gg = gamma.cuda().requires_grad_(True)
    bg = beta.cuda().requires_grad_(True)
    rg = resid.cuda().requires_grad_(True) if res else None
    if pad:             # padded-output kernels (k_gn_fwd_pad / k_gn_bwd_pad)
        assert relu and gn_pad_eligible(xg, G)
        y, y_pad = groupnorm_relu_pad(xg, C, G, gg, bg, res=rg)
        assert y_pad is not None and y_pad.shape[-2:] == (H + 2, W + 2)
    else:
        y = groupnorm_act(xg, C, G, gg, bg, res=rg, relu=relu)
    y.backward(dy.cuda())
    y_raw, mean, rstd = ops.groupnorm_fwd(
        x.cuda(), resid.cuda() if res else torch.empty(0, dtype=dtype,
                                                       device="cuda"),
        gamma.cuda(), beta.cuda(), C, G, 1e-5, relu)
    assert torch.equal(y_raw, y.detach())

    xv, gb, bb, dims, sdims = kb.gn_views(upcast(x), upcast(gamma),
                                          upcast(beta), C, G)
    rv = upcast(resid).reshape(xv.shape) if res else None
    dyv = upcast(dy).reshape(xv.shape)
    r = kb.norm_math(xv, gb, bb, dims, _f32(1e-5), res=rv)
    tag = "gnpad" if pad else f"gn{layout}"
    mask = None
    want_y = r["pre"]
    if relu:
        dec = kb.relu_decided(r["pre"], r["pre_scale"], n, dtype,
                              intrinsic=True, label=tag)
        mask = kb.relu_mask(r["pre"], dec, y.reshape(xv.shape))
        want_y = r["pre"].clamp_min(0)
    r = kb.norm_math(xv, gb, bb, dims, _f32(1e-5), res=rv, dy=dyv, mask=mask)

    assert_bounded(y.reshape(xv.shape), want_y, r["pre_scale"], n, dtype,
                   intrinsic=True, label=tag + ".y")
    assert_bounded(mean, r["mean"].reshape(-1), r["mean_scale"].reshape(-1),
                   n, F32, label=tag + ".mean")
    assert_bounded(rstd, r["rstd"].reshape(-1), r["rstd_scale"].reshape(-1),
                   n, F32, intrinsic=True, label=tag + ".rstd")
    assert_bounded(xg.grad.reshape(xv.shape), r["dx"], r["dx_scale"], n,
                   dtype, intrinsic=True, label=tag + ".dx")
    if res:
        assert_bounded(rg.grad.reshape(xv.shape), r["g"], r["g"].abs(), 1,
                       dtype, label=tag + ".dres")
    nred = B * HW
    assert_bounded(gg.grad, r["gx"].sum(sdims).reshape(C, ch),
                   r["gx_scale"].sum(sdims).reshape(C, ch), nred + n, dtype,
                   intrinsic=True, label=tag + ".dgamma")
    assert_bounded(bg.grad, r["g"].sum(sdims).reshape(C, ch),
                   r["g"].abs().sum(sdims).reshape(C, ch), nred, dtype,
                   label=tag + ".dbeta")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("relu,res", [(False, False), (True, False),
                                      (False, True), (True, True)])
@pytest.mark.parametrize("shape,layout", list(zip(GN_SHAPES, GN_LAYOUT)),
                         ids=[str(s) for s in GN_SHAPES])
def test_groupnorm_dense_bounded(shape, layout, relu, res, dtype):
    _check_groupnorm(shape, layout, relu, res, dtype)


@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("shape", [(1, 16, 1, 28, 28), (2, 16, 2, 4, 6),
                                   (2, 64, 2, 8, 8)], ids=str)
def test_groupnorm_padded_pair_bounded(shape, res):
    """The padded-output pair against fp64 directly (test_gn_pad_gpu.py
    compares it with the dense kernels bit for bit at power-of-two
    planes); 28x28 and 4x6 planes have a non-power-of-two vector count."""
    _check_groupnorm(shape, 1, True, res, BF, pad=True)


@pytest.mark.parametrize("dtype", DTYPES)
def test_groupnorm_shifted_mean_bounded(dtype):
    _check_groupnorm((2, 64, 2, 8, 8), 1, False, False, dtype, shift=True)


# ---------------------------------------------------------------------------
# fused SGD / FedProx and weighted delta accumulation

SIZES = [64, 15, 103, 7, 128]            # n % 8 in {0, 7}


def _layout(sizes, clients, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    offs = [0]
    for s in sizes:
        offs.append(offs[-1] + s)
    P = offs[-1]
    master = torch.randn(P, generator=g).to(dtype)
    buf = torch.randn(clients * P, generator=g).to(dtype)
    grad = torch.randn(clients * P, generator=g).to(dtype)
    return buf, grad, master, offs


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("mu", [0.0, 0.3])
@pytest.mark.parametrize("C", [1, 5, 130])
def test_fused_sgd_bounded(C, mu, dtype):
    from olearning_sim_amd.ops import fused
    buf, grad, master, offs = _layout(SIZES, C, dtype, 20 + C)
    ref, scale = kb.sgd_math(upcast(buf), upcast(grad), upcast(master), offs,
                             C, _f32(0.1), _f32(mu))
    out = buf.cuda()
    fused.fused_sgd_update_flat(out, grad.cuda(), master.cuda(), C, lr=0.1,
                                mu=mu, offsets=torch.tensor(
                                    offs, dtype=torch.int64).cuda())
    # w - lr*(g + mu*(w - m)): 4 roundings before the store
    assert_bounded(out, ref, scale, 4, dtype, label="sgd")


def _check_delta(sizes, C, dtype, seed):
    from olearning_sim_amd.ops import fused
    buf, _, master, offs = _layout(sizes, C, dtype, seed)
    g = torch.Generator().manual_seed(seed + 1)
    w = torch.rand(C, generator=g)
    delta = torch.randn(master.numel(), generator=g)
    wsum = float(w.sum())
    ref, _, scale_h = kb.delta_math(upcast(delta), upcast(buf),
                                    upcast(master), upcast(w), offs, C)
    out = delta.cuda()
    fused.weighted_delta_accum_flat(
        out, buf.cuda(), master.cuda(), w.cuda(), C,
        offsets=torch.tensor(offs, dtype=torch.int64).cuda(), wsum=wsum)
    # the kernels hoist the master term (sum_c w_c buf_c - wsum*master),
    # so the scale is that expression's (kernel_bounds.delta_math); wsum
    # arrives as an fp32 sum of C weights: C more terms
    assert_bounded(out, ref, scale_h, 2 * C + 1, F32, label="delta")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [1, 5, 130])
def test_delta_accum_blocks_bounded(C, dtype):
    _check_delta(SIZES, C, dtype, 40 + C)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", [1, 5, 130])
@pytest.mark.parametrize("n", [4096, 103])
def test_delta_accum_single_param_bounded(n, C, dtype):
    """nblocks == 1: bf16 takes k_delta_accum_v8 (n % 8 == 0), the
    client-parallel atomics kernels at C >= 64, else the generic one."""
    _check_delta([n], C, dtype, 60 + C)
