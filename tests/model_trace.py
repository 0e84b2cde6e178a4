"""Teacher-forced check of a whole ResNet-18 / LeNet step, call by call.

bf16 compounds over a network, so the models are not compared with fp64
end to end.  Instead a recording proxy (``TraceOps``, installed like the
``_CountingOps`` proxies: ``monkeypatch.setattr(fused, "_HIP_OPS", proxy)``)
keeps every extension call of one forward and backward pass with the very
tensors it received and returned, and

- ``check_calls`` compares each call with the fp64 reference of that one
  operation on the exact operands of the record, under the bound the
  per-kernel test of the entry point uses (``kernel_bounds``; no new error
  term), data movement exactly;
- ``check_resnet_flow`` / ``check_block`` / ``check_lenet_flow`` check the
  wiring between the calls by tensor identity (``data_ptr``): which
  activation each layer reads at which stride, which residual, that every
  parameter gradient autograd returns IS the output of that layer's
  gradient call, and that an activation with several consumers receives the
  bf16 sum of their recorded gradients.

Together: the model is the right network up to one bounded rounding per
operation.  A failure raises ``TraceFailure`` whose ``label`` names the
check (``<entry point>.<output>`` or ``flow.<what>``); the CPU file proves
each label sharp with mutants of a torch stand-in.  A call of an entry
point without a checker fails ("unchecked extension call"), so a new fused
op cannot enter the models unchecked."""

from __future__ import annotations

import torch
import torch.nn.functional as F

import kernel_bounds as kb
from kernel_bounds import upcast

BF, F32 = torch.bfloat16, torch.float32

# host-only queries pass through the proxy unrecorded
_HOST_NAMES = ("conv3x3_v6_ok", "gn_pad_ok")
_HOST_SUFFIXES = ("_route", "_tile", "_staging")


class TraceFailure(AssertionError):
    def __init__(self, label, msg):
        super().__init__(f"{label}: {msg}")
        self.label = label


class Call:
    """One recorded extension call; the tensors stay alive with it."""

    def __init__(self, idx, name, args, outs, route):
        self.idx, self.name, self.args, self.outs = idx, name, args, outs
        self.route = route          # conv calls: kernel of the shape, else None
        self.memo = {}              # fp64 intermediates a later checker reuses

    def __repr__(self):
        return f"<call {self.idx} {self.name}>"


def _f32(v):
    return float(torch.tensor(float(v), dtype=torch.float32))


def _ptr(t):
    return t.data_ptr()


def interior(t, p=1):
    return t[..., p:-p, p:-p]


def halo_is_zero(t, p=1):
    z = t.detach().cpu().float().clone()
    z[..., p:-p, p:-p] = 0
    return not bool((z != 0).any())


def _conv3_shape(name, a):
    """(dir, IC, OC, B, H, W, stride) of a conv3x3 call's launch."""
    if name in ("conv3x3_fwd_p", "conv3x3_fwd"):
        h = 2 if name.endswith("_p") else 0
        x, w, s = a
        return ("fwd", w.shape[2], w.shape[1], x.shape[2], x.shape[3] - h,
                x.shape[4] - h, s)
    if name in ("conv3x3_dgrad_p", "conv3x3_dgrad"):
        dy, w, H, W, s = a
        return ("dgrad", w.shape[2], w.shape[1], dy.shape[2], H, W, s)
    h = 2 if name.endswith("_p") else 0
    x, dy, s = a
    return ("wgrad", x.shape[1], dy.shape[1], x.shape[2], x.shape[3] - h,
            x.shape[4] - h, s)


class TraceOps:
    """The extension namespace with every kernel call recorded in order."""

    def __init__(self, ops):
        self._ops = ops
        self.calls = []

    def _route(self, name, a):
        ops = self._ops
        if name.startswith("conv3x3_") and name != "conv3x3_wflip":
            d, *shape = _conv3_shape(name, a)
            r = str(ops.conv3x3_route(d, *shape))
            if d == "fwd":
                return " ".join((r, str(ops.conv3x3_tile(d, *shape)),
                                 str(ops.conv3x3_staging(d, *shape))))
            if d == "dgrad":
                return r + " " + str(ops.conv3x3_staging(d, *shape))
            return r
        if name == "conv5x5_fwd":
            x, w = a[0], a[1]
            return str(ops.conv5x5_route("fwd", w.shape[2], w.shape[1],
                                         x.shape[3], x.shape[4]))
        if name == "conv5x5_dgrad":
            w, H, W = a[1], a[3], a[4]
            return str(ops.conv5x5_route("dgrad", w.shape[2], w.shape[1],
                                         H, W))
        if name == "conv5x5_wgrad":
            x, dy = a[0], a[1]
            return str(ops.conv5x5_route("wgrad", x.shape[1], dy.shape[1],
                                         x.shape[3], x.shape[4]))
        return None

    def __getattr__(self, name):
        fn = getattr(self._ops, name)
        if name in _HOST_NAMES or name.endswith(_HOST_SUFFIXES):
            return fn

        def recorded(*a):
            # the route is a function of the environment as it is now
            route = self._route(name, a)
            out = fn(*a)
            outs = tuple(out) if isinstance(out, (tuple, list)) else (out,)
            self.calls.append(Call(len(self.calls), name, a, outs, route))
            return out
        return recorded

    def count(self):
        n = {}
        for c in self.calls:
            n[c.name] = n.get(c.name, 0) + 1
        return n


# ---------------------------------------------------------------------------
# helpers

def _fail(cond, call, what, msg):
    if not cond:
        label = what if call is None else f"{call.name}.{what}"
        where = "" if call is None else f"call {call.idx}: "
        raise TraceFailure(label, where + msg)


def _bounded(call, what, got, ref, scale, n, dtype, **kw):
    label = what if call is None else f"{call.name}.{what}"
    try:
        return kb.assert_bounded(got, ref, scale, n, dtype,
                                 label="trace." + label, **kw)
    except TraceFailure:
        raise
    except AssertionError as e:
        where = "" if call is None else f"call {call.idx}: "
        raise TraceFailure(label, where + str(e)) from None


def _same(call, what, got, want, msg="differs from the exact result"):
    got, want = got.detach().cpu(), want.detach().cpu()
    ok = got.shape == want.shape and got.dtype == want.dtype \
        and torch.equal(got, want)
    _fail(ok, call, what, msg)


def _conv_one(which, x, w, dy, stride, pad, bias=None):
    """One of kernel_bounds.conv_all's three results."""
    if which == "y":
        return kb.conv_math(x, w, stride, pad, bias)
    with torch.enable_grad():       # also when called inside a backward
        xr = x.detach().clone().requires_grad_(which == "dx")
        wr = w.detach().clone().requires_grad_(which == "dw")
        y = kb.conv_math(xr, wr, stride, pad)
        return torch.autograd.grad(y, xr if which == "dx" else wr, dy)[0]


def conv_dir(which, x, w, dy, stride, pad, bias=None):
    """(reference, abs-value scale) as kernel_bounds.conv_ref forms them,
    for the one direction a call computes; fp64 operands."""
    ref = _conv_one(which, x, w, dy, stride, pad, bias)
    scale = _conv_one(which, x.abs(), w.abs(),
                      None if dy is None else dy.abs(), stride, pad,
                      None if bias is None else bias.abs())
    return ref, scale


# ---------------------------------------------------------------------------
# one checker per entry point

class TraceCheck:
    def __init__(self, trace):
        self.calls = list(trace.calls)
        self.out_of = {}            # data_ptr -> (call, slot)
        for c in self.calls:
            for slot, t in enumerate(c.outs):
                if torch.is_tensor(t) and t.numel() > 0:
                    self.out_of[_ptr(t)] = (c, slot)
        self.layers = {}            # filled by the flow checks

    # -- identity -----------------------------------------------------
    def named(self, *names):
        return [c for c in self.calls if c.name in names]

    def src(self, t):
        """Storage a tensor stands for: the operand of the pad2d call that
        produced it, else its own."""
        got = self.out_of.get(_ptr(t))
        if got is not None and got[0].name == "pad2d":
            return _ptr(got[0].args[0])
        return _ptr(t)

    def flipped_from(self, w):
        """The recorded conv3x3_wflip call that produced w, or None."""
        got = self.out_of.get(_ptr(w))
        return got[0] if got and got[0].name == "conv3x3_wflip" else None

    # -- conv3x3 ---------------------------------------------------------
    def _operand(self, call, t, padded, p=1):
        if not padded:
            return upcast(t)
        _fail(halo_is_zero(t, p), call, "operand_halo",
              "padded operand has a non-zero halo")
        return upcast(interior(t, p))

    def conv3x3_fwd(self, c):
        xp, w, s = c.args
        padded = c.name.endswith("_p")
        x = self._operand(c, xp, padded)
        ref, scale = conv_dir("y", x, upcast(w), None, s, 1)
        # forward kernel on flipped weights: the stride-1 dgrad.  Same
        # reference - the conv of the operand with the operand weights
        what = "dgrad_wt" if self.flipped_from(w) is not None else "y"
        _bounded(c, what, c.outs[0], ref, scale, w.shape[2] * 9, BF)

    def conv3x3_wflip(self, c):
        (w,) = c.args
        _same(c, "wt", c.outs[0],
              w.detach().cpu().flip(-1, -2).transpose(1, 2).contiguous())

    def conv3x3_dgrad(self, c):
        dyp, w, H, W, s = c.args
        dy = self._operand(c, dyp, c.name.endswith("_p"))
        C, OC, IC = w.shape[:3]
        x0 = torch.zeros(C, IC, dy.shape[2], H, W, dtype=torch.float64)
        ref, scale = conv_dir("dx", x0, upcast(w), dy, s, 1)
        _bounded(c, "dx", c.outs[0], ref, scale, OC * 9, BF)

    def conv3x3_wgrad(self, c):
        xp, dy, s = c.args
        x = self._operand(c, xp, c.name.endswith("_p"))
        C, OC = dy.shape[:2]
        w0 = torch.zeros(C, OC, x.shape[1], 3, 3, dtype=torch.float64)
        ref, scale = conv_dir("dw", x, w0, upcast(dy), s, 1)
        _bounded(c, "dw", c.outs[0], ref, scale,
                 dy.shape[2] * dy.shape[3] * dy.shape[4], BF)

    def pad2d(self, c):
        x, p = c.args
        _fail(halo_is_zero(c.outs[0], p), c, "halo", "halo is not zero")
        _same(c, "interior", interior(c.outs[0], p), x)

    # -- GroupNorm ---------------------------------------------------------
    def _gn_fwd_ref(self, c):
        """fp64 forward of a groupnorm_fwd / groupnorm_fwd_pad record."""
        if "r" in c.memo:
            return c.memo
        x, res, gamma, beta, clients, groups, eps, flag = c.args
        pad_api = c.name == "groupnorm_fwd_pad"
        relu = True if pad_api else bool(flag)
        pad_out = bool(flag) if pad_api else False
        xv, gb, bb, dims, sdims = kb.gn_views(upcast(x), upcast(gamma),
                                              upcast(beta), clients, groups)
        rv = None
        if res.numel() > 0:
            rv = self._operand(c, res, res.shape != x.shape)
            rv = rv.reshape(xv.shape)
        r = kb.norm_math(xv, gb, bb, dims, _f32(eps), res=rv)
        y = c.outs[0]
        yv = upcast(interior(y) if pad_out else y).reshape(xv.shape)
        ch = gamma.shape[-1]
        n = (ch // groups) * x.shape[-2] * x.shape[-1]
        dec = None
        if relu:
            try:
                dec = kb.relu_decided(r["pre"], r["pre_scale"], n, x.dtype,
                                      intrinsic=True,
                                      label=f"trace.{c.name}")
            except AssertionError as e:
                raise TraceFailure(c.name + ".undecided", str(e)) from None
        c.memo.update(r=r, rv=rv, yv=yv, n=n, dec=dec, relu=relu,
                      pad_out=pad_out, views=(xv, gb, bb, dims, sdims))
        return c.memo

    def groupnorm_fwd(self, c):
        m = self._gn_fwd_ref(c)
        r, n, x = m["r"], m["n"], c.args[0]
        if m["pad_out"]:
            _fail(halo_is_zero(c.outs[0]), c, "halo",
                  "halo of the padded output is not zero")
        # an undecided sign (|pre| within its own bound) passes either way
        want = r["pre"].clamp_min(0) if m["relu"] else r["pre"]
        _bounded(c, "y", m["yv"], want, r["pre_scale"], n, x.dtype,
                 intrinsic=True)
        mean, rstd = c.outs[-2], c.outs[-1]
        _bounded(c, "mean", mean, r["mean"].reshape(-1),
                 r["mean_scale"].reshape(-1), n, F32)
        _bounded(c, "rstd", rstd, r["rstd"].reshape(-1),
                 r["rstd_scale"].reshape(-1), n, F32, intrinsic=True)

    def _gn_fwd_of(self, c):
        """The forward record a backward call belongs to: same h, same
        mean."""
        x, mean = c.args[0], c.args[3]
        for f in self.named("groupnorm_fwd", "groupnorm_fwd_pad"):
            if _ptr(f.args[0]) == _ptr(x) and _ptr(f.outs[-2]) == _ptr(mean):
                return f
        _fail(False, c, "forward", "no forward call with this h and mean")

    def groupnorm_bwd(self, c):
        pad_api = c.name == "groupnorm_bwd_pad"
        if pad_api:
            x, _mask, dy, mean, rstd, gamma, clients, groups, has_res, \
                want_pad = c.args
            dx, dx_pad, dres, dgamma, dbeta = c.outs
        else:
            x, y_op, dy, mean, rstd, gamma, clients, groups, has_res, \
                relu_op = c.args
            dx, dres, dgamma, dbeta = c.outs
        f = self._gn_fwd_of(c)
        m = self._gn_fwd_ref(f)
        _fail(_ptr(f.outs[-1]) == _ptr(rstd) and _ptr(f.args[2]) == _ptr(gamma)
              and has_res == (f.args[1].numel() > 0), c, "operands",
              "rstd, gamma or has_res are not the forward call's")
        if not pad_api:
            _fail(_ptr(y_op) == _ptr(f.outs[0]) and bool(relu_op) == m["relu"],
                  c, "operands", "y or relu are not the forward call's")
        xv, gb, bb, dims, sdims = m["views"]
        # the mask is never decoded from the mask operand: fp64 sign where
        # decided, the sign of the FORWARD call's y elsewhere
        mask = kb.relu_mask(m["r"]["pre"], m["dec"], m["yv"]) \
            if m["relu"] else None
        r = kb.norm_math(xv, gb, bb, dims, _f32(f.args[6]), res=m["rv"],
                         dy=upcast(dy).reshape(xv.shape), mask=mask)
        n, dt = m["n"], x.dtype
        _bounded(c, "dx", upcast(dx).reshape(xv.shape), r["dx"],
                 r["dx_scale"], n, dt, intrinsic=True)
        if has_res:
            _bounded(c, "dres", upcast(dres).reshape(xv.shape), r["g"],
                     r["g"].abs(), 1, dt)
        else:
            _fail(dres.numel() == 0, c, "dres", "dres without a residual")
        C, ch = dgamma.shape
        B = x.shape[2] if x.dim() == 5 else x.shape[0]
        nred = B * x.shape[-2] * x.shape[-1]
        _bounded(c, "dgamma", dgamma, r["gx"].sum(sdims).reshape(C, ch),
                 r["gx_scale"].sum(sdims).reshape(C, ch), nred + n,
                 dgamma.dtype, intrinsic=True)
        _bounded(c, "dbeta", dbeta, r["g"].sum(sdims).reshape(C, ch),
                 r["g"].abs().sum(sdims).reshape(C, ch), nred, dbeta.dtype)
        if pad_api and want_pad:
            _fail(halo_is_zero(dx_pad), c, "dh_pad_halo",
                  "halo of dh_pad is not zero")
            _same(c, "dh_pad", interior(dx_pad), dx,
                  "interior of dh_pad is not dh")
        elif pad_api:
            _fail(dx_pad.numel() == 0, c, "dh_pad", "unrequested dh_pad")

    # -- subsample -----------------------------------------------------------
    def subsample2(self, c):
        x = c.args[0].detach().cpu()
        if c.name == "subsample2_p":
            x = interior(x)
        _same(c, "y", c.outs[0], x[..., ::2, ::2].contiguous())

    def subsample2_bwd(self, c):
        dy, H, W = c.args
        dy = dy.detach().cpu()
        want = torch.zeros(*dy.shape[:-2], H, W, dtype=dy.dtype)
        want[..., ::2, ::2] = dy
        _same(c, "dx", c.outs[0], want)

    # -- conv5x5, relu_mask, pool -------------------------------------------
    def conv5x5_fwd(self, c):
        x, w, b, _nt, relu = c.args
        x64, w64, b64 = upcast(x), upcast(w), upcast(b)
        pre, scale = conv_dir("y", x64, w64, None, 1, 0, b64)
        n = w.shape[2] * 25 + 1
        want = pre
        if relu:
            try:
                dec = kb.relu_decided(pre, scale, n, BF, label="trace.conv5")
            except AssertionError as e:
                raise TraceFailure(c.name + ".undecided", str(e)) from None
            c.memo["dec"] = dec
            want = pre.clamp_min(0)
        _bounded(c, "y", c.outs[0], want, scale, n, BF)

    def conv5x5_dgrad(self, c):
        dyp, w, _nt, H, W = c.args
        dy = self._operand(c, dyp, True, 4)
        C, OC, IC = w.shape[:3]
        x0 = torch.zeros(C, IC, dy.shape[2], H, W, dtype=torch.float64)
        ref, scale = conv_dir("dx", x0, upcast(w), dy, 1, 0)
        _bounded(c, "dx", c.outs[0], ref, scale, OC * 25, BF)

    def conv5x5_wgrad(self, c):
        x, dy, _nt = c.args
        C, OC = dy.shape[:2]
        w0 = torch.zeros(C, OC, x.shape[1], 5, 5, dtype=torch.float64)
        ref, scale = conv_dir("dw", upcast(x), w0, upcast(dy), 1, 0)
        _bounded(c, "dw", c.outs[0], ref, scale,
                 dy.shape[2] * dy.shape[3] * dy.shape[4], BF)

    def relu_mask(self, c):
        dy, y = (t.detach().cpu() for t in c.args)
        _same(c, "out", c.outs[0], dy * (y > 0).to(dy.dtype))

    @staticmethod
    def _windows(t):                        # [..., OH, OW, 4], 2*dh + dw
        H, W = t.shape[-2:]
        t = t.reshape(*t.shape[:-2], H // 2, 2, W // 2, 2)
        return t.transpose(-3, -2).reshape(*t.shape[:-4], H // 2, W // 2, 4)

    def pool2x2_fwd(self, c):
        x = c.args[0].detach().cpu()
        y, arg = (t.detach().cpu() for t in c.outs)
        xw = self._windows(x)
        _same(c, "y", y, xw.max(dim=-1).values)
        _fail(int(arg.max()) <= 3, c, "arg", "argmax code above 3")
        at = xw.gather(-1, arg.long().unsqueeze(-1)).squeeze(-1)
        _same(c, "arg", at, y, "x at the recorded argmax is not the maximum")

    def pool2x2_bwd(self, c):
        dy, arg = (t.detach().cpu() for t in c.args)
        hot = F.one_hot(arg.long(), 4).to(dy.dtype) * dy.unsqueeze(-1)
        OH, OW = dy.shape[-2:]
        want = hot.reshape(*dy.shape, 2, 2).transpose(-3, -2) \
            .reshape(*dy.shape[:-2], OH * 2, OW * 2)
        _same(c, "dx", c.outs[0], want)

    # -- the fc head ---------------------------------------------------------
    def transpose2d(self, c):
        _same(c, "y", c.outs[0],
              c.args[0].detach().cpu().transpose(1, 2).contiguous())

    def cross_entropy_fwd_bwd(self, c):
        logits, labels = c.args
        N, K = logits.shape
        ref = kb.ce_math(upcast(logits), labels.cpu())
        row, dl = c.outs
        _bounded(c, "row_loss", row, ref["row"], ref["row_scale"], K, F32,
                 intrinsic=True)
        _bounded(c, "dlogits", dl, ref["grad"], ref["grad_scale"], K,
                 logits.dtype, intrinsic=True)


CHECKERS = {
    "conv3x3_fwd_p": TraceCheck.conv3x3_fwd,
    "conv3x3_fwd": TraceCheck.conv3x3_fwd,
    "conv3x3_wflip": TraceCheck.conv3x3_wflip,
    "conv3x3_dgrad_p": TraceCheck.conv3x3_dgrad,
    "conv3x3_dgrad": TraceCheck.conv3x3_dgrad,
    "conv3x3_wgrad_p": TraceCheck.conv3x3_wgrad,
    "conv3x3_wgrad": TraceCheck.conv3x3_wgrad,
    "pad2d": TraceCheck.pad2d,
    "groupnorm_fwd": TraceCheck.groupnorm_fwd,
    "groupnorm_fwd_pad": TraceCheck.groupnorm_fwd,
    "groupnorm_bwd": TraceCheck.groupnorm_bwd,
    "groupnorm_bwd_pad": TraceCheck.groupnorm_bwd,
    "subsample2": TraceCheck.subsample2,
    "subsample2_p": TraceCheck.subsample2,
    "subsample2_bwd": TraceCheck.subsample2_bwd,
    "conv5x5_fwd": TraceCheck.conv5x5_fwd,
    "conv5x5_dgrad": TraceCheck.conv5x5_dgrad,
    "conv5x5_wgrad": TraceCheck.conv5x5_wgrad,
    "relu_mask": TraceCheck.relu_mask,
    "pool2x2_fwd": TraceCheck.pool2x2_fwd,
    "pool2x2_bwd": TraceCheck.pool2x2_bwd,
    "transpose2d": TraceCheck.transpose2d,
    "cross_entropy_fwd_bwd": TraceCheck.cross_entropy_fwd_bwd,
}


def check_calls(trace):
    """Run the checker of every recorded call, in call order.  Returns the
    TraceCheck for the flow checks."""
    tc = TraceCheck(trace)
    for c in tc.calls:
        if c.name not in CHECKERS:
            raise TraceFailure("unchecked", f"call {c.idx}: unchecked "
                               f"extension call {c.name}")
    for c in tc.calls:
        CHECKERS[c.name](tc, c)
    return tc


# ---------------------------------------------------------------------------
# dataflow between the calls

def _one(found, label, msg):
    if len(found) != 1:
        raise TraceFailure(label, f"{msg}: {len(found)} calls {found}")
    return found[0]


def check_accum(got, parts, what="flow.accum"):
    """``got`` (the dy operand of a producer's backward call, or what
    autograd returned for a leaf) against the recorded gradients of its k
    consumers: the tensor itself for k = 1, else their bf16 sum in any
    order - k - 1 roundings of partial sums no larger than sum |part| -
    against the fp64 sum."""
    k = len(parts)
    if k == 1:
        _same(None, what, got, parts[0],
              "gradient is not the single consumer's recorded gradient")
        return
    ref = sum(upcast(p) for p in parts)
    scale = sum(upcast(p).abs() for p in parts)
    _bounded(None, what, got, ref, scale, k, got.dtype, roundings=k - 1)


def check_conv_gn(tc, name, params, grads, x_in, stride, gn, res="none"):
    """One 3x3 layer ``name`` (weight params[name + '.w']) and the
    GroupNorm ``gn`` behind it.  x_in: the tensor the layer must read (a
    padded image, or the dense activation a recorded pad2d padded); None
    skips that.  res: "none", or the tensor the GroupNorm must add.
    Returns the calls; with grads, checks the backward wiring as well."""
    w = params[name + ".w"]
    gn_inputs = {_ptr(c.args[0])
                 for c in tc.named("groupnorm_fwd", "groupnorm_fwd_pad")}
    on_w = [c for c in tc.named("conv3x3_fwd_p", "conv3x3_fwd")
            if _ptr(c.args[1]) == _ptr(w)]
    fwd = _one([c for c in on_w if _ptr(c.outs[0]) in gn_inputs],
               "flow.conv_count", f"{name}: forward convs on this weight")
    if len(on_w) != 1:
        # the forward kernel is the stride-1 dgrad only on the FLIPPED copy
        raise TraceFailure("flow.dgrad", f"{name}: the forward kernel ran "
                           f"{len(on_w)} times on the unflipped weights")
    if x_in is not None and tc.src(fwd.args[0]) != tc.src(x_in):
        raise TraceFailure("flow.input", f"{name} reads another activation")
    if fwd.args[2] != stride:
        raise TraceFailure("flow.stride", f"{name} ran at stride "
                           f"{fwd.args[2]}, expected {stride}")
    g, b = params[gn + ".g"], params[gn + ".b"]
    gnf = _one([c for c in tc.named("groupnorm_fwd", "groupnorm_fwd_pad")
                if _ptr(c.args[0]) == _ptr(fwd.outs[0])], "flow.gn_input",
               f"{gn}: GroupNorm calls on the output of {name}")
    if _ptr(gnf.args[2]) != _ptr(g) or _ptr(gnf.args[3]) != _ptr(b):
        raise TraceFailure("flow.gn_params", f"{gn}: other gamma / beta")
    r = gnf.args[1]
    if (res == "none") != (r.numel() == 0) or \
            (r.numel() > 0 and tc.src(r) != tc.src(res)):
        raise TraceFailure("flow.residual", f"{gn}: wrong residual operand")
    out = {"fwd": fwd, "gn": gnf, "gnb": None, "dgrad": None, "wgrad": None}
    tc.layers[name] = out
    if grads is None:
        return out
    gnb = _one([c for c in tc.named("groupnorm_bwd", "groupnorm_bwd_pad")
                if _ptr(c.args[0]) == _ptr(gnf.args[0])], "flow.gn_bwd",
               f"{gn}: backward calls")
    dh, dgamma, dbeta = gnb.outs[0], gnb.outs[-2], gnb.outs[-1]
    _same(None, "flow.gn_grads", grads[gn + ".g"], dgamma.to(g.dtype),
          f"{gn}.g: autograd's gradient is not the call's dgamma")
    _same(None, "flow.gn_grads", grads[gn + ".b"], dbeta.to(b.dtype),
          f"{gn}.b: autograd's gradient is not the call's dbeta")
    wg = _one([c for c in tc.named("conv3x3_wgrad_p", "conv3x3_wgrad")
               if _ptr(c.args[0]) == _ptr(fwd.args[0])], "flow.wgrad",
              f"{name}: wgrad calls on the layer's input")
    if _ptr(wg.args[1]) != _ptr(dh) or wg.args[2] != stride:
        raise TraceFailure("flow.wgrad", f"{name}: wgrad not on dh of {gn}")
    _same(None, "flow.wgrad", grads[name + ".w"], wg.outs[0],
          f"{name}.w: autograd's gradient is not the wgrad call's output")
    dg = [c for c in tc.named("conv3x3_dgrad_p", "conv3x3_dgrad")
          if _ptr(c.args[1]) == _ptr(w)]
    for c in tc.named("conv3x3_fwd_p"):
        flip = tc.flipped_from(c.args[1])
        if flip is not None and _ptr(flip.args[0]) == _ptr(w):
            dg.append(c)
    # a dgrad on anything else - the unflipped weights run through the
    # forward kernel, say - shows as a layer without one
    out.update(gnb=gnb, wgrad=wg)
    if dg or x_in is not None:
        d = _one(dg, "flow.dgrad", f"{name}: dgrad calls on this weight "
                 "(or its recorded flipped copy)")
        ok = {_ptr(t) for t in gnb.outs[:2] if t.numel() > 0}
        if tc.src(d.args[0]) not in ok:
            raise TraceFailure("flow.dgrad", f"{name}: dgrad not on dh")
        if d.name != "conv3x3_fwd_p" and d.args[4] != stride:
            raise TraceFailure("flow.dgrad", f"{name}: dgrad stride")
        out["dgrad"] = d
    return out


def check_block(tc, params, grads, pre, x_in, stride, has_down, pad_out):
    """One residual block ``pre`` on the activation x_in.  Returns (last
    GroupNorm forward call, its backward call, the recorded gradients of
    the block input's consumers)."""
    l1 = check_conv_gn(tc, pre + ".c1", params, grads, x_in, stride,
                       pre + ".gn1")
    h1 = l1["gn"].outs[0]
    if has_down:
        sub = _one([c for c in tc.named("subsample2", "subsample2_p")
                    if tc.src(c.args[0]) == tc.src(x_in)], "flow.subsample",
                   f"{pre}: subsample calls on the block input")
        gd, bd = params[pre + ".gndown.g"], params[pre + ".gndown.b"]
        gnd = _one([c for c in tc.named("groupnorm_fwd", "groupnorm_fwd_pad")
                    if _ptr(c.args[2]) == _ptr(gd)
                    and _ptr(c.args[3]) == _ptr(bd)], "flow.gn_params",
                   f"{pre}.gndown: GroupNorm calls")
        if gnd.args[1].numel() or (gnd.name == "groupnorm_fwd"
                                   and gnd.args[7]):
            raise TraceFailure("flow.residual", f"{pre}.gndown: residual "
                               "or ReLU on the shortcut")
        # the 1x1 conv is torch's bmm: test_conv1x1_bounded's bound
        wd = upcast(params[pre + ".down.w"])
        C, OC, IC = wd.shape[:3]
        wd = wd.reshape(C, OC, IC)
        xs = upcast(sub.outs[0])
        flat = xs.reshape(C, IC, -1)
        sc = gnd.args[0]
        _bounded(None, "flow.down", upcast(sc).reshape(C, OC, -1),
                 torch.bmm(wd, flat), torch.bmm(wd.abs(), flat.abs()), IC,
                 sc.dtype)
        res = gnd.outs[0]
    else:
        res = x_in
    l2 = check_conv_gn(tc, pre + ".c2", params, grads, h1, 1, pre + ".gn2",
                       res=res)
    gn2 = l2["gn"]
    if gn2.name == "groupnorm_fwd_pad" and bool(gn2.args[7]) != pad_out:
        raise TraceFailure("flow.pad_out", f"{pre}: pad_out is "
                           f"{gn2.args[7]}, expected {pad_out}")
    if grads is None:
        return gn2, None, None
    # h1 has the one consumer c2
    check_accum(l1["gnb"].args[2], [l2["dgrad"].outs[0]])
    dres = l2["gnb"].outs[-3]
    parts = [l1["dgrad"].outs[0]]
    if has_down:
        gndb = _one([c for c in tc.named("groupnorm_bwd", "groupnorm_bwd_pad")
                     if _ptr(c.args[0]) == _ptr(gnd.args[0])], "flow.gn_bwd",
                    f"{pre}.gndown: backward calls")
        check_accum(gndb.args[2], [dres])
        _same(None, "flow.gn_grads", grads[pre + ".gndown.g"],
              gndb.outs[-2].to(gd.dtype), f"{pre}.gndown.g")
        _same(None, "flow.gn_grads", grads[pre + ".gndown.b"],
              gndb.outs[-1].to(bd.dtype), f"{pre}.gndown.b")
        dsc = upcast(gndb.outs[0]).reshape(C, OC, -1)
        sb = _one([c for c in tc.named("subsample2_bwd")
                   if tuple(c.outs[0].shape[:3]) == tuple(xs.shape[:3])
                   and c.outs[0].shape[-1] == 2 * xs.shape[-1]],
                  "flow.subsample", f"{pre}: subsample2_bwd calls")
        _bounded(None, "flow.down_dx", upcast(sb.args[0]).reshape(C, IC, -1),
                 torch.bmm(wd.transpose(1, 2), dsc),
                 torch.bmm(wd.abs().transpose(1, 2), dsc.abs()), OC, BF)
        _bounded(None, "flow.down_dw",
                 upcast(grads[pre + ".down.w"]).reshape(C, OC, IC),
                 torch.bmm(dsc, flat.transpose(1, 2)),
                 torch.bmm(dsc.abs(), flat.abs().transpose(1, 2)),
                 flat.shape[-1], BF)
        parts.append(sb.outs[0])
    else:
        parts.append(dres)
    return gn2, l2["gnb"], parts


def resnet_blocks(names):
    """[(prefix, stride, has_down)] from the parameter names as
    init_global generates them (not from forward_cbf)."""
    pres = sorted({n[:-len(".c1.w")] for n in names if n.endswith(".c1.w")})
    out = []
    for pre in pres:
        s, b = int(pre[1]), int(pre[4])
        out.append((pre, 2 if s > 0 and b == 0 else 1,
                    pre + ".down.w" in names))
    return out


def check_resnet_flow(tc, params, grads, x):
    """Stem, eight blocks and the gradient sums between them."""
    stem = check_conv_gn(tc, "stem", params, grads, None, 1, "stem.gn")
    _same(None, "flow.input", stem["fwd"].args[0],
          x.permute(0, 2, 1, 3, 4).contiguous(),
          "the stem does not read the [C, 3, B, H, W] input")
    if stem["dgrad"] is not None:
        raise TraceFailure("flow.dgrad", "the stem has no input gradient")
    prev_f, prev_b = stem["gn"], stem["gnb"]
    blocks = resnet_blocks(list(params))
    for i, (pre, stride, has_down) in enumerate(blocks):
        f, b, parts = check_block(tc, params, grads, pre, prev_f.outs[0],
                                  stride, has_down, i < len(blocks) - 1)
        check_accum(prev_b.args[2], parts)
        prev_f, prev_b = f, b
    return tc


def check_lenet_flow(tc, params, grads, x):
    """conv1 -> pool -> conv2 -> pool -> [C, B, 400] -> fc1, and back."""
    prev = None
    convs = []
    for name in ("conv1", "conv2"):
        w, b = params[name + ".w"], params[name + ".b"]
        cv = _one([c for c in tc.named("conv5x5_fwd")
                   if _ptr(c.args[1]) == _ptr(w)], "flow.conv_count",
                  f"{name}: forward calls")
        if _ptr(cv.args[2]) != _ptr(b) or not cv.args[4]:
            raise TraceFailure("flow.conv_params", f"{name}: bias or ReLU")
        if prev is None:
            _same(None, "flow.input", cv.args[0],
                  x.permute(0, 2, 1, 3, 4).contiguous(),
                  "conv1 does not read the [C, 3, B, H, W] input")
        elif _ptr(cv.args[0]) != _ptr(prev.outs[0]):
            raise TraceFailure("flow.input", f"{name} reads another tensor")
        pool = _one([c for c in tc.named("pool2x2_fwd")
                     if _ptr(c.args[0]) == _ptr(cv.outs[0])], "flow.pool",
                    f"{name}: pool calls on its output")
        convs.append((name, cv, pool))
        tc.layers[name] = {"fwd": cv, "dgrad": None, "wgrad": None}
        prev = pool
    C, B = x.shape[:2]
    want = prev.outs[0].detach().cpu().permute(0, 2, 1, 3, 4) \
        .reshape(C, B, 400)
    fc1 = [c for c in tc.named("transpose2d")
           if tuple(c.args[0].shape) == (C, B, 400)]
    _one(fc1, "flow.fc1_input", "transposes of the fc1 input")
    _same(None, "flow.fc1_input", fc1[0].args[0], want,
          "fc1 does not receive the [C, B, 400] rearrangement")
    if grads is None:
        return tc
    nxt = None                              # dgrad call of the layer above
    for name, cv, pool in reversed(convs):
        pb = _one([c for c in tc.named("pool2x2_bwd")
                   if _ptr(c.args[1]) == _ptr(pool.outs[1])], "flow.pool",
                  f"{name}: pool backward calls")
        if nxt is not None:
            check_accum(pb.args[0], [nxt.outs[0]])
        rm = _one([c for c in tc.named("relu_mask")
                   if _ptr(c.args[1]) == _ptr(cv.outs[0])], "flow.relu_mask",
                  f"{name}: relu_mask calls on its output")
        check_accum(rm.args[0], [pb.outs[0]])
        dy = rm.outs[0]
        wg = _one([c for c in tc.named("conv5x5_wgrad")
                   if _ptr(c.args[0]) == _ptr(cv.args[0])], "flow.wgrad",
                  f"{name}: wgrad calls")
        if _ptr(wg.args[1]) != _ptr(dy):
            raise TraceFailure("flow.wgrad", f"{name}: wgrad not on the "
                               "masked gradient")
        _same(None, "flow.wgrad", grads[name + ".w"], wg.outs[0],
              f"{name}.w: autograd's gradient is not the wgrad output")
        # db is a torch sum of the masked gradient
        dy64 = upcast(dy)
        _bounded(None, "flow.dbias", grads[name + ".b"],
                 dy64.sum(dim=(2, 3, 4)), dy64.abs().sum(dim=(2, 3, 4)),
                 dy.shape[2] * dy.shape[3] * dy.shape[4], BF)
        dg = [c for c in tc.named("conv5x5_dgrad")
              if _ptr(c.args[1]) == _ptr(params[name + ".w"])]
        tc.layers[name]["wgrad"] = wg
        if name == "conv1":
            if dg:
                raise TraceFailure("flow.dgrad", "conv1 has no input "
                                   "gradient")
            continue
        nxt = _one(dg, "flow.dgrad", f"{name}: dgrad calls")
        if tc.src(nxt.args[0]) != _ptr(dy):
            raise TraceFailure("flow.dgrad", f"{name}: dgrad not on the "
                               "masked gradient")
        tc.layers[name]["dgrad"] = nxt
    return tc


def route_table(tc):
    """{layer: (fwd, dgrad, wgrad)} routes of the layers the flow checks
    identified; the flipped-weight dgrad is a forward call and reports the
    forward kernel of the swapped shape, prefixed "wt:"."""
    out = {}
    for name, l in tc.layers.items():
        d = l["dgrad"]
        dr = None if d is None else \
            ("wt:" + d.route if d.name == "conv3x3_fwd_p" else d.route)
        out[name] = (l["fwd"].route, dr,
                     None if l["wgrad"] is None else l["wgrad"].route)
    return out


# ---------------------------------------------------------------------------
# the cases (shared by the GPU tests and the CPU check of the references)

GN_GROUPS = 8


def draw_params(model, C, seed):
    """Per-client bf16 parameters, on the CPU.  gamma = 1 + 0.1 randn and
    beta = 0.1 randn: init_global's ones and zeros would hide a dropped
    gamma or beta.  Every other tensor differs per client by 5 %."""
    gen = torch.Generator().manual_seed(seed)
    out = {}
    for k, v in model.init_global(generator=gen).items():
        rep = v.float().unsqueeze(0).expand(C, *v.shape).clone()
        noise = torch.randn(rep.shape, generator=gen)
        if "gn" in k and k.endswith(".g"):
            rep = 1 + 0.1 * noise
        elif "gn" in k and k.endswith(".b"):
            rep = 0.1 * noise
        else:
            rep = rep * (1 + 0.05 * noise)
        out[k] = rep.to(BF)
    return out, gen


def model_inputs(model, C, B, gen):
    x = torch.randn((C, B) + tuple(model.input_shape), generator=gen).to(BF)
    y = torch.randint(0, model.num_classes, (C, B), generator=gen)
    return x, y


def resnet_case(width_mult=0.5, C=2, B=2, seed=31):
    from olearning_sim_amd.models import build_model
    m = build_model("resnet18", num_classes=10, width_mult=width_mult)
    params, gen = draw_params(m, C, seed)
    return (m, params) + model_inputs(m, C, B, gen)


def lenet_case(C=3, B=8, seed=32):
    from olearning_sim_amd.models import build_model
    m = build_model("lenet")
    params, gen = draw_params(m, C, seed)
    return (m, params) + model_inputs(m, C, B, gen)


LAST_STAGE = (("s3.b0", 2, True), ("s3.b1", 1, False))


def last_stage_case(C=1, B=2, seed=33):
    """The full-width s3.b0 (256 -> 512, stride 2 from 8x8, with down) and
    s3.b1 (512 -> 512 at 4x4, padded residual, dense output) alone: K =
    2304 and 4608, ch/G = 64.  Returns the model, the two blocks'
    parameters, a random dense input [C, 256, B, 8, 8] (the caller pads
    it) and a random upstream gradient [C, 512, B, 4, 4]."""
    from olearning_sim_amd.models import build_model
    m = build_model("resnet18", num_classes=10, width_mult=1.0)
    params, gen = draw_params(m, C, seed)
    params = {k: v for k, v in params.items() if k.startswith("s3.")}
    x = torch.randn(C, 256, B, 8, 8, generator=gen).clamp_min(0).to(BF)
    dy = (0.1 * torch.randn(C, 512, B, 4, 4, generator=gen)).to(BF)
    return m, params, x, dy
