"""Padded-output GroupNorm pair vs the existing kernels composed.

The reference for everything here is what the dense path runs today:
ops.groupnorm_fwd -> ops.pad2d, ops.groupnorm_bwd -> ops.pad2d and
ops.subsample2.  The padded kernels keep the same arithmetic and the same
reduction order, so every comparison is bit-exact (atol=0, rtol=0); only
dgamma/dbeta at B > 2 (more than two atomic adds per channel) use the
tolerances of test_groupnorm_fused_matches_reference."""

import pytest
import torch

pytestmark = pytest.mark.gpu

G = 8
EPS = 1e-5

# [C, ch, B, H, W]
SHAPES = [
    (3, 16, 2, 4, 4),      # fewer vectors than threads, 36-element plane
    (2, 64, 1, 8, 8),
    (1, 128, 1, 16, 16),
    (1, 64, 2, 32, 32),    # full stage-0 plane
    (1, 16, 1, 4, 8),      # H != W catches swapped strides
]
RES_MODES = ["none", "dense", "padded"]


@pytest.fixture(scope="module")
def ops():
    from olearning_sim_amd.ops import load_hip_ops
    return load_hip_ops(required=True)


def _exact(a, b):
    torch.testing.assert_close(a, b, atol=0, rtol=0)


def _inputs(shape, seed=0):
    C, ch, B, H, W = shape
    g = torch.Generator().manual_seed(seed)
    bf = torch.bfloat16
    x = torch.randn(shape, generator=g).to(bf).cuda()
    res = torch.randn(shape, generator=g).to(bf).cuda()
    dy = torch.randn(shape, generator=g).to(bf).cuda()
    gamma = (1 + 0.1 * torch.randn(C, ch, generator=g)).to(bf).cuda()
    beta = (0.1 * torch.randn(C, ch, generator=g)).to(bf).cuda()
    return x, res, dy, gamma, beta


def _sentinel(shape_padded):
    """Best effort at making an unwritten halo visible: the op allocates
    its own output, so park a non-zero pattern in a block of the same
    size and free it for the caching allocator to hand back."""
    t = torch.full(shape_padded, 7.0, dtype=torch.bfloat16, device="cuda")
    del t


def _run_pair(ops, shape, res_mode):
    """(reference dict, padded-kernel dict) for one shape / residual mode."""
    C, ch, B, H, W = shape
    x, res, dy, gamma, beta = _inputs(shape)
    has_res = res_mode != "none"
    empty = torch.empty(0, dtype=x.dtype, device=x.device)
    y, mean, rstd = ops.groupnorm_fwd(x, res if has_res else empty, gamma,
                                      beta, C, G, EPS, True)
    assert 0.2 < (y > 0).float().mean().item() < 0.8   # non-trivial mask
    dx, dres, dgamma, dbeta = ops.groupnorm_bwd(x, y, dy, mean, rstd, gamma,
                                                C, G, has_res, True)
    ref = dict(y=y, y_pad=ops.pad2d(y, 1), mean=mean, rstd=rstd, dx=dx,
               dx_pad=ops.pad2d(dx, 1), dres=dres, dgamma=dgamma,
               dbeta=dbeta)

    if res_mode == "none":
        res_arg = empty
    elif res_mode == "dense":
        res_arg = res
    else:
        res_arg = ops.pad2d(res, 1)
    _sentinel((C, ch, B, H + 2, W + 2))
    y_pad, mask, mean2, rstd2 = ops.groupnorm_fwd_pad(
        x, res_arg, gamma, beta, C, G, EPS, True)
    y_dense, mask_d, _, _ = ops.groupnorm_fwd_pad(
        x, res_arg, gamma, beta, C, G, EPS, False)
    _sentinel((C, ch, B, H + 2, W + 2))
    dx2, dx_pad2, dres2, dgamma2, dbeta2 = ops.groupnorm_bwd_pad(
        x, mask, dy, mean2, rstd2, gamma, C, G, has_res, True)
    dx3, dx_pad3, _, _, _ = ops.groupnorm_bwd_pad(
        x, mask_d, dy, mean2, rstd2, gamma, C, G, has_res, False)
    new = dict(y=y_dense, y_pad=y_pad, mean=mean2, rstd=rstd2, dx=dx2,
               dx_pad=dx_pad2, dres=dres2, dgamma=dgamma2, dbeta=dbeta2,
               dx_nopad=dx3, dx_pad_none=dx_pad3, mask=mask, mask_d=mask_d)
    return ref, new


@pytest.mark.parametrize("res_mode", RES_MODES)
@pytest.mark.parametrize("shape", SHAPES)
def test_gn_pad_matches_dense_then_pad(ops, shape, res_mode):
    C, ch, B, H, W = shape
    assert ops.gn_pad_ok(ch, G, H, W)
    ref, new = _run_pair(ops, shape, res_mode)
    assert new["y_pad"].shape == (C, ch, B, H + 2, W + 2)
    _exact(new["mean"], ref["mean"])
    _exact(new["rstd"], ref["rstd"])
    _exact(new["y_pad"], ref["y_pad"])          # halo included
    _exact(new["y"], ref["y"])                  # dense-output variant
    assert torch.equal(new["mask"], new["mask_d"])
    _exact(new["dx"], ref["dx"])
    _exact(new["dx_pad"], ref["dx_pad"])        # halo included
    _exact(new["dx_nopad"], ref["dx"])
    assert new["dx_pad_none"].numel() == 0
    if res_mode != "none":
        _exact(new["dres"], ref["dres"])
    else:
        assert new["dres"].numel() == 0
    # B <= 2: at most two commutative atomic adds per channel
    assert B <= 2
    _exact(new["dgamma"], ref["dgamma"])
    _exact(new["dbeta"], ref["dbeta"])


def test_gn_pad_dgamma_large_batch(ops):
    """B > 2: the per-channel atomics are order-dependent, so dgamma and
    dbeta are checked against an fp32 torch reference with the
    tolerances test_groupnorm_fused_matches_reference uses; the
    deterministic outputs stay bit-exact."""
    from olearning_sim_amd.ops.fused import groupnorm_act
    shape = (2, 16, 4, 4, 4)
    C, ch, B, H, W = shape
    ref, new = _run_pair(ops, shape, "padded")
    _exact(new["y_pad"], ref["y_pad"])
    _exact(new["dx"], ref["dx"])
    _exact(new["dx_pad"], ref["dx_pad"])
    _exact(new["dres"], ref["dres"])
    x, res, dy, gamma, beta = _inputs(shape)
    xr = x.float().cpu()
    gr = gamma.float().cpu().requires_grad_(True)
    br = beta.float().cpu().requires_grad_(True)
    yr = groupnorm_act(xr, C, G, gr, br, res=res.float().cpu(), relu=True,
                       eps=EPS)
    yr.backward(dy.float().cpu())
    torch.testing.assert_close(new["dgamma"].cpu(), gr.grad, atol=2e-1,
                               rtol=5e-2)
    torch.testing.assert_close(new["dbeta"].cpu(), br.grad, atol=2e-1,
                               rtol=5e-2)


def test_gn_pad_autograd_pair(ops):
    """groupnorm_relu_pad returns (interior view, padded image); grads
    arrive dense and equal the dense op's."""
    from olearning_sim_amd.ops.fused import groupnorm_act, groupnorm_relu_pad
    shape = (2, 64, 1, 8, 8)
    C = shape[0]
    x, res, dy, gamma, beta = _inputs(shape, seed=3)
    outs = []
    for fn in ("pad", "dense"):
        xs = [t.detach().clone().requires_grad_(True)
              for t in (x, res, gamma, beta)]
        if fn == "pad":
            y, y_pad = groupnorm_relu_pad(xs[0], C, G, xs[2], xs[3],
                                          res=xs[1])
            assert y_pad is not None and not y_pad.requires_grad
            assert y.data_ptr() != y_pad.data_ptr() and y._base is y_pad
        else:
            y = groupnorm_act(xs[0], C, G, xs[2], xs[3], res=xs[1],
                              relu=True)
        outs.append((y,) + torch.autograd.grad(y, xs, dy))
    for a, b in zip(*outs):
        _exact(a, b)


def test_gn_pad_fallback_when_backward_does_not_fit(ops):
    """(1, 256, 1, 32, 32): the forward staging fits 64 KB, the backward's
    (x + masked dy) does not, so the pair takes the dense kernels."""
    from olearning_sim_amd.ops.fused import groupnorm_relu_pad
    shape = (1, 256, 1, 32, 32)
    C, ch, B, H, W = shape
    assert (ch // G) * H * W * 2 <= 65536 < (ch // G) * H * W * 4
    assert not ops.gn_pad_ok(ch, G, H, W)
    x, res, dy, gamma, beta = _inputs(shape)
    y_ref, mean, rstd = ops.groupnorm_fwd(x, res, gamma, beta, C, G, EPS,
                                          True)
    dx_ref, dres_ref, _, _ = ops.groupnorm_bwd(x, y_ref, dy, mean, rstd,
                                               gamma, C, G, True, True)
    xg = x.detach().clone().requires_grad_(True)
    rg = res.detach().clone().requires_grad_(True)
    y, y_pad = groupnorm_relu_pad(xg, C, G, gamma, beta, res=rg)
    assert y_pad is None
    _exact(y, y_ref)
    dx, dres = torch.autograd.grad(y, [xg, rg], dy)
    _exact(dx, dx_ref)
    _exact(dres, dres_ref)


@pytest.mark.parametrize("shape", [(2, 32, 2, 8, 8), (1, 32, 1, 4, 8)])
def test_subsample2_padded_input(ops, shape):
    g = torch.Generator().manual_seed(1)
    x = torch.randn(shape, generator=g).to(torch.bfloat16).cuda()
    _exact(ops.subsample2_p(ops.pad2d(x, 1)), ops.subsample2(x))


def test_resnet_gn_pad_bit_equal_to_dense_path(ops, monkeypatch):
    """ResNet18(width_mult=0.5), C=2, B=2: loss and every parameter
    gradient bit-equal between OLSIM_GN_PAD=0 and the default."""
    from olearning_sim_amd.models import build_model
    from olearning_sim_amd.engine.client_manager import (FlatParams,
                                                         replicate_params)
    from olearning_sim_amd.ops import conv as conv_mod
    m = build_model("resnet18", num_classes=100, width_mult=0.5)
    gen = torch.Generator().manual_seed(0)
    gp = {k: v.cuda() for k, v in m.init_global(generator=gen).items()}
    master = FlatParams(gp)
    C, B = 2, 2
    x = torch.randn(C, B, 3, 32, 32, generator=gen).to(torch.bfloat16).cuda()
    y = torch.randint(0, 100, (C, B), generator=gen).cuda()

    pads = []
    real_pad = conv_mod._pad
    monkeypatch.setattr(conv_mod, "_pad",
                        lambda t, p: (pads.append(1), real_pad(t, p))[1])

    def run():
        params = replicate_params(master.cast(torch.bfloat16), C)
        names = list(params)
        loss = m.loss(params, x, y)
        grads = torch.autograd.grad(loss, [params[k] for k in names])
        assert all(g is not None for g in grads)
        return loss.detach(), dict(zip(names, grads))

    monkeypatch.setenv("OLSIM_GN_PAD", "0")
    loss0, g0 = run()
    assert len(pads) == 32          # 16 padded convs, x and dy each
    del pads[:]
    monkeypatch.delenv("OLSIM_GN_PAD")
    loss1, g1 = run()
    assert not pads                 # no pad pass left on the padded path
    _exact(loss1, loss0)
    for k in g0:
        _exact(g1[k], g0[k])
