"""Every extension call of a ResNet-18 / LeNet training step against fp64
(tests/model_trace.py): the call on the exact operands the network handed
it, under the bound of its per-kernel test, plus the wiring between the
calls, the call counts and the kernel every conv layer reached.

Each case runs one forward and backward pass on the GPU once; the tests
that check its calls and its wiring share the trace."""

import pytest
import torch
import torch.nn.functional as F

import model_trace as mt

pytestmark = pytest.mark.gpu

ENVS = {"default": {}, "gn_pad0": {"OLSIM_GN_PAD": "0"},
        "dgrad_wt0": {"OLSIM_DGRAD_WT": "0"}}
SWITCHES = ("OLSIM_GN_PAD", "OLSIM_DGRAD_WT", "OLSIM_CONV", "OLSIM_CONV_V",
            "OLSIM_CONV_DW64", "OLSIM_CONV_DW8", "OLSIM_CONV_NMAJOR",
            "OLSIM_CONV_BM64", "OLSIM_CONV5", "OLSIM_PAD", "OLSIM_BMM_SAFE")


@pytest.fixture(scope="module", autouse=True)
def _require_ext():
    from olearning_sim_amd.ops import load_hip_ops
    load_hip_ops(required=True)


_RUNS: dict = {}


def _traced(key, env, step):
    """Run step() once per key under the recording proxy and the given
    switches; the trace (and with it every tensor) is kept for the tests
    that share it."""
    if key not in _RUNS:
        from olearning_sim_amd.ops import fused
        with pytest.MonkeyPatch.context() as mp:
            for var in SWITCHES:
                mp.delenv(var, raising=False)
            for var, val in env.items():
                mp.setenv(var, val)
            trace = mt.TraceOps(fused.load_hip_ops(required=True))
            mp.setattr(fused, "_HIP_OPS", trace)
            _RUNS[key] = (trace,) + step()
            torch.cuda.synchronize()
    return _RUNS[key]


def _model_step(case):
    m, p0, x, y = case
    p = {k: v.cuda().requires_grad_(True) for k, v in p0.items()}
    x, y = x.cuda(), y.cuda()
    loss = m.loss(p, x, y)
    names = list(p)
    grads = dict(zip(names, torch.autograd.grad(loss, [p[k] for k in names])))
    return p, grads, x


def _resnet_run(env):
    return _traced("resnet." + env, ENVS[env],
                   lambda: _model_step(mt.resnet_case()))


# ---------------------------------------------------------------------------
# expected routes, read off the launchers' branches by hand (conv3_route.h:
# fwd_v7 at stride 1, OW >= 8 and IC*9 % 64 == 0, else fwd_v6<lg OW, stride>;
# 128x64 where OC is a multiple of 128; k-major at stride 1 except
# fwd_v7<3,1>; wgrad_v8 / v8s at OW >= 8; the flipped-weight dgrad "wt:" is
# the forward of the swapped shape), not produced by conv3x3_route.
# layer -> (fwd, dgrad, wgrad)

def _stage(fwd, wgrad):
    return (fwd, "wt:" + fwd, wgrad)


S0 = _stage("fwd_v6<4,1> 64x128 kmajor", "wgrad_v8")
S1 = _stage("fwd_v7<4,1> 64x128 kmajor", "wgrad_v8")
S2 = _stage("fwd_v7<3,1> 128x64 nmajor", "wgrad_v8")
S3 = _stage("fwd_v6<2,1> 128x64 kmajor", "wgrad_v6")
# ResNet18(0.5): 32 / 64 / 128 / 256 channels at 32 / 16 / 8 / 4, C = B = 2
HALF_ROUTES = {
    # IC = 3: K = 27, the v5 family; no input gradient
    "stem": ("fwd_v2 64x128 nmajor", None, "wgrad_v5"),
    "s0.b0.c1": S0, "s0.b0.c2": S0, "s0.b1.c1": S0, "s0.b1.c2": S0,
    "s1.b0.c1": ("fwd_v6<4,2> 64x128 nmajor", "dgrad_s2<4> nmajor",
                 "wgrad_v8s"),
    "s1.b0.c2": S1, "s1.b1.c1": S1, "s1.b1.c2": S1,
    "s2.b0.c1": ("fwd_v6<3,2> 128x64 nmajor", "dgrad_s2<3> nmajor",
                 "wgrad_v8s"),
    "s2.b0.c2": S2, "s2.b1.c1": S2, "s2.b1.c2": S2,
    "s3.b0.c1": ("fwd_v6<2,2> 128x64 nmajor", "dgrad_s2<2> nmajor",
                 "wgrad_v6"),
    "s3.b0.c2": S3, "s3.b1.c1": S3, "s3.b1.c2": S3,
}
# OLSIM_DGRAD_WT=0: the stride-1 dgrads run dgrad_v6<lg OW> (k-major)
DGRAD_V6 = {"s0": "dgrad_v6<4> kmajor", "s1": "dgrad_v6<4> kmajor",
            "s2": "dgrad_v6<3> kmajor", "s3": "dgrad_v6<2> kmajor"}
# full width: 256 -> 512 from 8x8 at stride 2, then 512 -> 512 at 4x4
LAST_STAGE_ROUTES = {"s3.b0.c1": HALF_ROUTES["s3.b0.c1"], "s3.b0.c2": S3,
                     "s3.b1.c1": S3, "s3.b1.c2": S3}
LENET_ROUTES = {"conv1": ("direct", None, "mfma"),
                "conv2": ("direct", "direct", "mfma")}

HEAD = {"transpose2d": 2, "cross_entropy_fwd_bwd": 1}
COUNTS = {
    # 17 conv forwards (the stem dense) + 13 stride-1 dgrads on flipped
    # copies; the 3 strided c1 keep dgrad_s2; no pad2d pass
    "default": dict(HEAD, conv3x3_fwd=1, conv3x3_wgrad=1, conv3x3_fwd_p=29,
                    conv3x3_wflip=13, conv3x3_dgrad_p=3, conv3x3_wgrad_p=16,
                    groupnorm_fwd_pad=17, groupnorm_bwd_pad=17,
                    groupnorm_fwd=3, groupnorm_bwd=3, subsample2_p=3,
                    subsample2_bwd=3),
    # dense GroupNorm everywhere, x and dy of the 16 padded convs through
    # pad2d, the shortcut subsamples the dense activation
    "gn_pad0": dict(HEAD, conv3x3_fwd=1, conv3x3_wgrad=1, conv3x3_fwd_p=29,
                    conv3x3_wflip=13, conv3x3_dgrad_p=3, conv3x3_wgrad_p=16,
                    groupnorm_fwd=20, groupnorm_bwd=20, pad2d=32,
                    subsample2=3, subsample2_bwd=3),
    # no repack, every dgrad through conv3x3_dgrad_p
    "dgrad_wt0": dict(HEAD, conv3x3_fwd=1, conv3x3_wgrad=1, conv3x3_fwd_p=16,
                      conv3x3_dgrad_p=16, conv3x3_wgrad_p=16,
                      groupnorm_fwd_pad=17, groupnorm_bwd_pad=17,
                      groupnorm_fwd=3, groupnorm_bwd=3, subsample2_p=3,
                      subsample2_bwd=3),
}


def _print_routes(title, routes):
    print(f"routes[{title}]")
    for name, r in routes.items():
        print(f"  {name}: {r}")


@pytest.mark.parametrize("env", list(ENVS))
def test_resnet18_every_call_bounded(env):
    """ResNet18(width_mult=0.5), num_classes=10, C = 2, B = 2, loss through
    m.loss and one autograd.grad over all parameters: every recorded call
    against fp64.  (The fp64 references of one run take 0.3 s, so the case
    is not split by stage.)"""
    mt.check_calls(_resnet_run(env)[0])


@pytest.mark.parametrize("env", list(ENVS))
def test_resnet18_wiring_counts_and_routes(env):
    trace, p, grads, x = _resnet_run(env)
    assert trace.count() == COUNTS[env], trace.count()
    tc = mt.TraceCheck(trace)
    mt.check_resnet_flow(tc, p, grads, x)
    want = dict(HALF_ROUTES)
    if env == "dgrad_wt0":
        want = {k: (f, DGRAD_V6[k[:2]] if d and d.startswith("wt:") else d, w)
                for k, (f, d, w) in want.items()}
    got = mt.route_table(tc)
    _print_routes("resnet18(0.5)." + env, got)
    assert got == want


def _last_stage_step():
    m, p0, x, dy = mt.last_stage_case()
    p = {k: v.cuda().requires_grad_(True) for k, v in p0.items()}
    xd = x.cuda().requires_grad_(True)
    x_pad = F.pad(xd.detach(), (1, 1, 1, 1))
    h, h_pad = xd, x_pad
    for i, (pre, stride, has_down) in enumerate(mt.LAST_STAGE):
        h, h_pad = m._block_cbf(p, h, h_pad, x.shape[0], pre, stride,
                                has_down, pad_out=i == 0)
    assert h_pad is None
    names = list(p)
    g = torch.autograd.grad(h, [xd] + [p[k] for k in names], dy.cuda())
    return p, dict(zip(names, g[1:])), (x_pad, g[0], dy)


def test_last_stage_full_width_every_call_bounded():
    """_block_cbf for s3.b0 and s3.b1 at full width, C = 1, B = 2: K = 2304
    and 4608, two M tiles and more, ch/G = 64."""
    mt.check_calls(_traced("last_stage", {}, _last_stage_step)[0])


def test_last_stage_full_width_wiring_counts_and_routes():
    trace, p, grads, (x_pad, dx, dy) = _traced("last_stage", {},
                                               _last_stage_step)
    assert trace.count() == dict(
        conv3x3_fwd_p=4 + 3, conv3x3_wflip=3, conv3x3_dgrad_p=1,
        conv3x3_wgrad_p=4, groupnorm_fwd_pad=4, groupnorm_bwd_pad=4,
        groupnorm_fwd=1, groupnorm_bwd=1, subsample2_p=1, subsample2_bwd=1)
    tc = mt.TraceCheck(trace)
    f0, b0, parts0 = mt.check_block(tc, p, grads, "s3.b0", x_pad, 2, True,
                                    True)
    mt.check_accum(dx, parts0)
    f1, b1, parts1 = mt.check_block(tc, p, grads, "s3.b1", f0.outs[0], 1,
                                    False, False)
    mt.check_accum(b0.args[2], parts1)
    mt.check_accum(b1.args[2], [dy])
    got = mt.route_table(tc)
    _print_routes("resnet18(1.0) s3", got)
    assert got == LAST_STAGE_ROUTES


def test_lenet_every_call_bounded_and_wired():
    """LeNet, C = 3, B = 8 (conv2 needs B*100 % 32 == 0)."""
    trace, p, grads, x = _traced("lenet", {},
                                 lambda: _model_step(mt.lenet_case()))
    assert trace.count() == dict(
        conv5x5_fwd=2, pool2x2_fwd=2, pool2x2_bwd=2, relu_mask=2,
        conv5x5_wgrad=2, conv5x5_dgrad=1, pad2d=1, transpose2d=6,
        cross_entropy_fwd_bwd=1), trace.count()
    tc = mt.check_calls(trace)
    mt.check_lenet_flow(tc, p, grads, x)
    got = mt.route_table(tc)
    _print_routes("lenet", got)
    assert got == LENET_ROUTES
