"""CPU proof that the call-by-call model check (tests/model_trace.py) is
sharp: a plain-torch stand-in of the extension - fp32 arithmetic on the
bf16 operands, outputs rounded to bf16 - is driven through the real
autograd Function classes under the recording proxy.  Its traces must pass
every checker and the dataflow checks, and each mutant must fail with the
label of the check meant to catch it.  The last tests check the references
alone: at every GroupNorm and conv5x5 of the GPU cases the fp64 model's own
pre-activations keep the undecided ReLU share under relu_decided's cap."""

import pytest
import torch
import torch.nn.functional as F

import kernel_bounds as kb
import model_trace as mt
from model_trace import BF, interior

G = mt.GN_GROUPS
EPS = 1e-5


def _p2(v):
    return v > 0 and v & (v - 1) == 0


class StandIn:
    """Torch stand-in of the entry points a ResNet / LeNet step calls.
    ``mutant`` names one deliberate error."""

    def __init__(self, mutant=None):
        self.mutant = mutant

    # -- host queries, answered in Python --------------------------------
    def conv3x3_v6_ok(self, IC, OC, B, H, W, s):
        OH, OW = -(-H // s), -(-W // s)
        return (_p2(OH) and _p2(OW) and OW >= 4
                and not (s == 2 and (H | W) & 1) and IC * 9 % 32 == 0
                and OC * 9 % 32 == 0 and not (s == 2 and OC % 32)
                and s in (1, 2) and B * OH * OW % 32 == 0)

    def gn_pad_ok(self, ch, groups, H, W):
        return True

    def conv3x3_route(self, *a):
        return "standin"

    conv3x3_tile = conv3x3_staging = conv5x5_route = conv3x3_route

    # -- conv3x3 ---------------------------------------------------------
    @staticmethod
    def _grad(which, x, w, dy, s, pad):
        return mt._conv_one(which, x.float(), w.float(), dy.float(), s, pad)

    def conv3x3_fwd_p(self, xp, w, s):
        x = interior(xp).float()
        if self.mutant == "conv_s2_odd" and s == 2:
            return kb.conv_math(x, w.float(), 1, 1)[..., 1::2, 1::2] \
                .contiguous().to(BF)
        return kb.conv_math(x, w.float(), s, 1).to(BF)

    def conv3x3_wflip(self, w):
        return w.flip(-1, -2).transpose(1, 2).contiguous()

    def conv3x3_dgrad_p(self, dyp, w, H, W, s):
        C, OC, IC = w.shape[:3]
        x0 = torch.zeros(C, IC, dyp.shape[2], H, W)
        return self._grad("dx", x0, w, interior(dyp), s, 1).to(BF)

    def conv3x3_wgrad_p(self, xp, dy, s):
        x = interior(xp)
        if self.mutant == "wgrad_no_offset":
            x = xp[..., :-2, :-2]
        w0 = torch.zeros(dy.shape[0], dy.shape[1], x.shape[1], 3, 3)
        return self._grad("dw", x, w0, dy, s, 1).to(BF)

    def pad2d(self, x, p):
        return F.pad(x, (p, p, p, p))

    def transpose2d(self, x):
        return x.transpose(1, 2).contiguous()

    # -- GroupNorm -------------------------------------------------------
    def _gn(self, x, res, gamma, beta, clients, groups, eps, dy=None,
            mask=None):
        xv, gb, bb, dims, sdims = kb.gn_views(x.float(), gamma.float(),
                                              beta.float(), clients, groups)
        rv = None
        if res is not None and res.numel() > 0:
            rv = (res if res.shape == x.shape else interior(res)).float() \
                .reshape(xv.shape)
        if dy is not None:
            dy = dy.float().reshape(xv.shape)
            mask = None if mask is None else mask.reshape(xv.shape)
        return kb.norm_math(xv, gb, bb, dims, eps, res=rv, dy=dy,
                            mask=mask), sdims

    def groupnorm_fwd(self, x, res, gamma, beta, clients, groups, eps, relu):
        r, _ = self._gn(x, res, gamma, beta, clients, groups, eps)
        y = r["pre"].clamp_min(0) if relu else r["pre"]
        return (y.reshape(x.shape).to(x.dtype), r["mean"].reshape(-1),
                r["rstd"].reshape(-1))

    def groupnorm_fwd_pad(self, x, res, gamma, beta, clients, groups, eps,
                          pad_out):
        if self.mutant == "gn_ignores_res":
            res = None
        y, mean, rstd = self.groupnorm_fwd(x, res, gamma, beta, clients,
                                           groups, eps, True)
        mask = y > 0                         # any format: never decoded
        if pad_out:
            y = F.pad(y, (1, 1, 1, 1))
            if self.mutant == "y_halo":
                y[..., 0, 0] = 1.0
        return y, mask, mean, rstd

    def _gn_bwd(self, x, mask, dy, gamma, clients, groups, has_res):
        r, sdims = self._gn(x, None, gamma, torch.zeros_like(gamma), clients,
                            groups, EPS, dy=dy, mask=mask)
        C, ch = gamma.shape
        dres = r["g"].reshape(x.shape).to(x.dtype) if has_res \
            else x.new_empty(0)
        return (r["dx"].reshape(x.shape).to(x.dtype), dres,
                r["gx"].sum(sdims).reshape(C, ch),
                r["g"].sum(sdims).reshape(C, ch))

    def groupnorm_bwd(self, x, y, dy, mean, rstd, gamma, clients, groups,
                      has_res, relu):
        return self._gn_bwd(x, y > 0 if relu else None, dy, gamma, clients,
                            groups, has_res)

    def groupnorm_bwd_pad(self, x, mask, dy, mean, rstd, gamma, clients,
                          groups, has_res, want_pad):
        dx, dres, dgamma, dbeta = self._gn_bwd(x, mask, dy, gamma, clients,
                                               groups, has_res)
        if self.mutant == "dres_unmasked" and has_res:
            dres = dy.contiguous().clone()
        dx_pad = x.new_empty(0)
        if want_pad:
            src = torch.roll(dx, 1, -1) if self.mutant == "dh_shift" else dx
            dx_pad = F.pad(src, (1, 1, 1, 1))
            if self.mutant == "dh_halo":
                dx_pad[..., -1, -1] = 1.0
        return dx, dx_pad, dres, dgamma, dbeta

    # -- subsample -------------------------------------------------------
    def subsample2_p(self, xp):
        o = 1 if self.mutant == "sub_odd" else 0
        return interior(xp)[..., o::2, o::2].contiguous()

    def subsample2_bwd(self, dy, H, W):
        dx = dy.new_zeros(*dy.shape[:-2], H, W)
        dx[..., ::2, ::2] = dy
        return dx

    # -- conv5x5, relu_mask, pool ------------------------------------------
    def conv5x5_fwd(self, x, w, b, nt, relu):
        bias = None if self.mutant == "conv5_no_bias" else b.float()
        y = kb.conv_math(x.float(), w.float(), 1, 0, bias)
        return (y.clamp_min(0) if relu else y).to(BF)

    def conv5x5_dgrad(self, dyp, w, nt, H, W):
        C, OC, IC = w.shape[:3]
        x0 = torch.zeros(C, IC, dyp.shape[2], H, W)
        return self._grad("dx", x0, w, interior(dyp, 4), 1, 0).to(BF)

    def conv5x5_wgrad(self, x, dy, nt):
        w0 = torch.zeros(dy.shape[0], dy.shape[1], x.shape[1], 5, 5)
        return self._grad("dw", x, w0, dy, 1, 0).to(BF)

    def relu_mask(self, dy, y):
        keep = y >= 0 if self.mutant == "relu_ge" else y > 0
        return dy * keep.to(dy.dtype)

    def pool2x2_fwd(self, x):
        v, a = mt.TraceCheck._windows(x).max(dim=-1)
        return v.contiguous(), a.to(torch.uint8)

    def pool2x2_bwd(self, dy, arg):
        a = arg.long()
        if self.mutant == "pool_bwd_wrong":
            a = (a + 1) % 4
        hot = F.one_hot(a, 4).to(dy.dtype) * dy.unsqueeze(-1)
        OH, OW = dy.shape[-2:]
        return hot.reshape(*dy.shape, 2, 2).transpose(-3, -2) \
            .reshape(*dy.shape[:-2], OH * 2, OW * 2).contiguous()


# ---------------------------------------------------------------------------
# the traces: stem -> block without down -> block with a stride-2 down,
# through the real Function classes (they do not look at is_cuda)

BLOCKS = (("s0.b0", 1, False), ("s1.b0", 2, True))
C, B = 2, 2


def _resnet_inputs():
    g = torch.Generator().manual_seed(5)

    def rnd(*shape, s=1.0):
        return (s * torch.randn(*shape, generator=g)).to(BF)

    p = {"stem.w": rnd(C, 32, 32, 3, 3, s=0.08)}
    gns = {"stem.gn": 32}
    for pre, ic, oc in (("s0.b0", 32, 32), ("s1.b0", 32, 64)):
        p[pre + ".c1.w"] = rnd(C, oc, ic, 3, 3, s=0.08)
        p[pre + ".c2.w"] = rnd(C, oc, oc, 3, 3, s=0.06)
        gns[pre + ".gn1"] = gns[pre + ".gn2"] = oc
        if ic != oc:
            p[pre + ".down.w"] = rnd(C, oc, ic, 1, 1, s=0.2)
            gns[pre + ".gndown"] = oc
    for name, ch in gns.items():
        p[name + ".g"] = (1 + 0.1 * torch.randn(C, ch, generator=g)).to(BF)
        p[name + ".b"] = rnd(C, ch, s=0.1)
    return p, rnd(C, 32, B, 8, 8), rnd(C, 64, B, 4, 4, s=0.1)


def _run_resnet(monkeypatch, mutant=None, patch=None):
    from olearning_sim_amd.ops import conv, fused
    trace = mt.TraceOps(StandIn(mutant))
    monkeypatch.setattr(fused, "_HIP_OPS", trace)
    if patch is not None:
        patch(monkeypatch, conv)
    p0, x0, dy = _resnet_inputs()
    p = {k: v.clone().requires_grad_(True) for k, v in p0.items()}
    h = conv._Conv3x3PadFn.apply(x0, p["stem.w"], 1)
    h, h_pad = fused._GroupNormPadFn.apply(h, None, None, p["stem.gn.g"],
                                           p["stem.gn.b"], C, G, EPS)
    for i, (pre, stride, has_down) in enumerate(BLOCKS):
        x, x_pad = h, h_pad
        h, h_pad = conv._Conv3x3GnPadFn.apply(
            x, x_pad, p[pre + ".c1.w"], None, None, p[pre + ".gn1.g"],
            p[pre + ".gn1.b"], C, G, EPS, stride, True)
        if has_down:
            w = p[pre + ".down.w"]
            xs = conv._Subsample2PadFn.apply(x, x_pad)
            sc = torch.bmm(w.reshape(C, w.shape[1], w.shape[2]),
                           xs.reshape(C, w.shape[2], -1)) \
                .view(C, w.shape[1], *xs.shape[2:])
            sc = fused._GroupNormActFn.apply(
                sc, None, p[pre + ".gndown.g"], p[pre + ".gndown.b"], C, G,
                EPS, False)
            sc_pad = None
        else:
            sc, sc_pad = x, x_pad
        h, h_pad = conv._Conv3x3GnPadFn.apply(
            h, h_pad, p[pre + ".c2.w"], sc, sc_pad, p[pre + ".gn2.g"],
            p[pre + ".gn2.b"], C, G, EPS, 1, i < len(BLOCKS) - 1)
    names = list(p)
    grads = dict(zip(names, torch.autograd.grad(h, [p[k] for k in names],
                                                dy)))
    return trace, p, grads


def _check_resnet(trace, p, grads):
    tc = mt.check_calls(trace)
    stem = mt.check_conv_gn(tc, "stem", p, grads, None, 1, "stem.gn")
    prev_f, prev_b = stem["gn"], stem["gnb"]
    for i, (pre, stride, has_down) in enumerate(BLOCKS):
        f, b, parts = mt.check_block(tc, p, grads, pre, prev_f.outs[0],
                                     stride, has_down, i < len(BLOCKS) - 1)
        mt.check_accum(prev_b.args[2], parts)
        prev_f, prev_b = f, b
    return tc


def _run_conv5(monkeypatch, mutant=None):
    from olearning_sim_amd.ops import conv, fused
    trace = mt.TraceOps(StandIn(mutant))
    monkeypatch.setattr(fused, "_HIP_OPS", trace)
    g = torch.Generator().manual_seed(6)
    x = (0.5 * torch.randn(3, 6, 8, 14, 14, generator=g)).to(BF)
    w = (0.1 * torch.randn(3, 16, 6, 5, 5, generator=g)).to(BF)
    b = (0.1 * torch.randn(3, 16, generator=g)).to(BF)
    dy = (0.1 * torch.randn(3, 16, 8, 5, 5, generator=g)).to(BF)
    leaves = [t.requires_grad_(True) for t in (x, w, b)]
    y = conv._Pool2x2Fn.apply(conv._Conv5x5Fn.apply(*leaves, True))
    torch.autograd.grad(y, leaves, dy)
    return trace


def test_stand_in_traces_pass_every_check(monkeypatch):
    trace, p, grads = _run_resnet(monkeypatch)
    n = trace.count()
    assert n == {"conv3x3_fwd_p": 5 + 3, "conv3x3_wflip": 3,
                 "conv3x3_dgrad_p": 1, "conv3x3_wgrad_p": 5,
                 "groupnorm_fwd_pad": 5, "groupnorm_bwd_pad": 5,
                 "groupnorm_fwd": 1, "groupnorm_bwd": 1, "subsample2_p": 1,
                 "subsample2_bwd": 1}, n
    tc = _check_resnet(trace, p, grads)
    assert set(tc.layers) == {"stem", "s0.b0.c1", "s0.b0.c2", "s1.b0.c1",
                              "s1.b0.c2"}
    assert tc.layers["s1.b0.c1"]["dgrad"].name == "conv3x3_dgrad_p"
    assert tc.layers["s1.b0.c2"]["dgrad"].name == "conv3x3_fwd_p"
    trace = _run_conv5(monkeypatch)
    assert trace.count() == {"conv5x5_fwd": 1, "pool2x2_fwd": 1,
                             "pool2x2_bwd": 1, "relu_mask": 1,
                             "conv5x5_dgrad": 1, "conv5x5_wgrad": 1}
    # the relu_ge mutant needs exact zeros under a non-zero gradient
    rm = [c for c in trace.calls if c.name == "relu_mask"][0]
    assert bool(((rm.args[1] == 0) & (rm.args[0] != 0)).any())
    mt.check_calls(trace)


def test_unknown_entry_point_is_an_unchecked_call(monkeypatch):
    class Extra(StandIn):
        def fused_new_op(self, x):
            return x + 1

    trace = mt.TraceOps(Extra())
    trace.fused_new_op(torch.zeros(2))
    trace.gn_pad_ok(32, 8, 4, 4)
    trace.conv3x3_route("fwd", 32, 32, 2, 8, 8, 1)
    assert [c.name for c in trace.calls] == ["fused_new_op"]
    with pytest.raises(mt.TraceFailure, match="unchecked extension call"):
        mt.check_calls(trace)


def _swap_dres_into_x_slot(monkeypatch, conv):
    orig = conv._Conv3x3GnPadFn.backward

    def backward(ctx, dy, dyp):
        out = list(orig(ctx, dy, dyp))
        if out[3] is not None and out[0].shape == out[3].shape:
            out[0], out[3] = out[3], out[0]
        return tuple(out)
    monkeypatch.setattr(conv._Conv3x3GnPadFn, "backward",
                        staticmethod(backward))


def _zero_one_contribution(monkeypatch, conv):
    orig = conv._Conv3x3GnPadFn.backward

    def backward(ctx, dy, dyp):
        out = list(orig(ctx, dy, dyp))
        if out[3] is not None:              # after the call was recorded
            out[3] = torch.zeros_like(out[3])
        return tuple(out)
    monkeypatch.setattr(conv._Conv3x3GnPadFn, "backward",
                        staticmethod(backward))


def _dgrad_on_unflipped_weights(monkeypatch, conv):
    orig = conv._dgrad_p

    def dgrad(ops, dy_pad, w, H, W, stride, held=None):
        if stride == 1 and w.shape[1] == w.shape[2]:
            return ops.conv3x3_fwd_p(dy_pad, w, 1)
        return orig(ops, dy_pad, w, H, W, stride, held)
    monkeypatch.setattr(conv, "_dgrad_p", dgrad)


# mutant -> label of the check meant to catch it
RESNET_MUTANTS = {
    "gn_ignores_res": "groupnorm_fwd_pad.y",
    "dres_unmasked": "groupnorm_bwd_pad.dres",
    "y_halo": "groupnorm_fwd_pad.halo",
    "dh_halo": "groupnorm_bwd_pad.dh_pad_halo",
    "dh_shift": "groupnorm_bwd_pad.dh_pad",
    "conv_s2_odd": "conv3x3_fwd_p.y",
    "sub_odd": "subsample2_p.y",
    "wgrad_no_offset": "conv3x3_wgrad_p.dw",
}
RESNET_PATCHES = {
    "dgrad_on_unflipped_weights": (_dgrad_on_unflipped_weights, "flow.dgrad"),
    # c2's x is gn1's output, its residual the block input or the shortcut
    "dres_in_x_slot": (_swap_dres_into_x_slot, "flow.accum"),
    "one_contribution_zeroed": (_zero_one_contribution, "flow.accum"),
}
CONV5_MUTANTS = {
    "pool_bwd_wrong": "pool2x2_bwd.dx",
    "relu_ge": "relu_mask.out",
    "conv5_no_bias": "conv5x5_fwd.y",
}


@pytest.mark.parametrize("mutant", list(RESNET_MUTANTS))
def test_kernel_mutant_fails_its_checker(mutant, monkeypatch):
    trace, p, grads = _run_resnet(monkeypatch, mutant)
    with pytest.raises(mt.TraceFailure) as e:
        _check_resnet(trace, p, grads)
    assert e.value.label == RESNET_MUTANTS[mutant], str(e.value)


@pytest.mark.parametrize("mutant", list(RESNET_PATCHES))
def test_wiring_mutant_fails_the_flow_check(mutant, monkeypatch):
    patch, label = RESNET_PATCHES[mutant]
    trace, p, grads = _run_resnet(monkeypatch, patch=patch)
    mt.check_calls(trace)           # every call on its own is still right
    with pytest.raises(mt.TraceFailure) as e:
        _check_resnet(trace, p, grads)
    assert e.value.label == label, str(e.value)


@pytest.mark.parametrize("mutant", list(CONV5_MUTANTS))
def test_conv5_pool_mutant_fails_its_checker(mutant, monkeypatch):
    trace = _run_conv5(monkeypatch, mutant)
    with pytest.raises(mt.TraceFailure) as e:
        mt.check_calls(trace)
    assert e.value.label == CONV5_MUTANTS[mutant], str(e.value)


# ---------------------------------------------------------------------------
# the references alone: undecided ReLU share of the GPU cases

def _watch_groupnorm(monkeypatch, seen):
    """Every ReLU GroupNorm of a CPU fp64 forward through relu_decided,
    which asserts the cap max(0.1 %, 2 rel)."""
    from olearning_sim_amd.ops import fused
    orig = fused.groupnorm_act

    def watched(x, clients, groups, gamma, beta, res=None, relu=False,
                eps=1e-5):
        if relu:
            xv, gb, bb, dims, _ = kb.gn_views(x, gamma, beta, clients, groups)
            r = kb.norm_math(xv, gb, bb, dims, mt._f32(eps),
                             res=None if res is None else res.reshape(xv.shape))
            n = xv.shape[-3] * xv.shape[-2] * xv.shape[-1]
            kb.relu_decided(r["pre"], r["pre_scale"], n, BF, intrinsic=True,
                            label=f"gn {tuple(x.shape)}")
            seen.append(n)
        return orig(x, clients, groups, gamma, beta, res=res, relu=relu,
                    eps=eps)
    monkeypatch.setattr(fused, "groupnorm_act", watched)


def test_resnet_reference_keeps_relu_signs_decided(monkeypatch):
    """Seed 31 (resnet_case) and 33 (last_stage_case): every one of the 17
    and 4 ReLU GroupNorms stays under the cap."""
    seen = []
    _watch_groupnorm(monkeypatch, seen)
    m, params, x, _ = mt.resnet_case()
    m.forward({k: v.double() for k, v in params.items()}, x.double())
    assert len(seen) == 17
    del seen[:]
    m, params, x, _ = mt.last_stage_case()
    p64 = {k: v.double() for k, v in params.items()}
    Cc, ch, Bb, H, W = x.shape
    h = x.double().permute(2, 0, 1, 3, 4).reshape(Bb, Cc * ch, H, W)
    for pre, stride, has_down in mt.LAST_STAGE:
        h = m._block(p64, h, Cc, pre, stride, has_down)
    assert seen == [64 * 16] * 4


def test_lenet_reference_keeps_relu_signs_decided(monkeypatch):
    """Seed 32 (lenet_case): both fused conv5x5 ReLUs under the cap."""
    from olearning_sim_amd.models import lenet
    orig = lenet.bconv2d
    seen = []

    def watched(x, w, clients, b=None, stride=1, padding=0):
        pre = orig(x, w, clients, b, stride, padding)
        scale = orig(x.abs(), w.abs(), clients, b.abs(), stride, padding)
        kb.relu_decided(pre, scale, w.shape[2] * 25 + 1, BF,
                        label=f"conv5 {tuple(w.shape)}")
        seen.append(w.shape[2])
        return pre
    monkeypatch.setattr(lenet, "bconv2d", watched)
    m, params, x, _ = mt.lenet_case()
    m.forward({k: v.double() for k, v in params.items()}, x.double())
    assert seen == [3, 6]
