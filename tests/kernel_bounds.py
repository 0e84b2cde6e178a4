"""Derived element-wise error bounds for kernel-vs-fp64 comparisons.

Every numerics test of a HIP kernel compares the kernel output with an
fp64 reference computed from ``upcast`` copies of the exact tensors the
kernel received, and accepts

    |got - ref| <= roundings*u_out*|ref| + (n+2)*2^-23*scale
                   + intrinsic*2^-16*scale + 2^-126

- ``u_out``: 2^-8 for a bf16 output: bf16 carries 8 significant bits, so
  2^-8 is exactly ONE round-to-nearest (a lone rounding is observed at up
  to 0.996 of it).  2^-22 for an fp32 output (4 roundings).  A result
  that is rounded to bf16 twice - the cross-entropy gradient is stored
  in bf16 and then multiplied by the upstream gradient in bf16 - passes
  ``roundings=2``.
- ``scale``: the same operation evaluated on absolute values in fp64
  (``conv(|x|, |w|)``, ``|xhat||gamma| + |beta| + |res|``, ...).
- ``n``: the reduction length.  ``(n+2)*2^-23*scale`` is the textbook
  worst case of an fp32 sum of n terms in ANY order (atomics, trees,
  MFMA chains alike); the unit is 2^-23 rather than 2^-24 because MFMA
  accumulation may truncate instead of rounding to nearest.
- ``intrinsic``: ``__expf`` / ``__logf`` / ``rsqrtf``.  Fast exp loses
  about 2^-19 relative through its argument scaling at |x - max| <= 30;
  2^-16 is 8x over that.
- ``2^-126``: the flush-to-zero floor of fp32 and bf16 (both have 8
  exponent bits).  No kernel output can carry a magnitude below it, so a
  reference value of 1e-70 (softmax tail at logits +-80) is legitimately
  returned as 0.

These numbers are derived, not fitted: a kernel that exceeds them is a
finding.  The module also holds the dtype-generic math of the checked
operations, run in fp64 as the reference and (by the CPU tests) in fp32
as a stand-in kernel that the bound must accept and whose mutants it
must reject.
"""

from __future__ import annotations

import torch
import torch.nn.functional as F

U_OUT = {torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -22}
U_ACC = 2.0 ** -23
U_INTRINSIC = 2.0 ** -16
FTZ_FLOOR = 2.0 ** -126

# worst err/bound ratio seen per label in this process (information only)
HEADROOM: dict = {}


def upcast(t: torch.Tensor) -> torch.Tensor:
    """fp64 CPU copy of the exact tensor a kernel received."""
    return t.detach().to(device="cpu", dtype=torch.float64)


def bound(ref, scale, n, out_dtype, intrinsic=False, roundings=1):
    rel = (n + 2) * U_ACC + (U_INTRINSIC if intrinsic else 0.0)
    return (roundings * U_OUT[out_dtype] * ref.abs() + rel * scale
            + FTZ_FLOOR)


def assert_bounded(got, ref, scale, n, out_dtype, intrinsic=False,
                   where=None, label="", roundings=1):
    """Assert |got - ref| <= bound element-wise (optionally only ``where``).
    Returns the worst error as a fraction of its bound."""
    got = upcast(got)
    ref = ref.to(torch.float64)
    scale = torch.as_tensor(scale, dtype=torch.float64)
    assert got.shape == ref.shape, (label, tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all()), f"{label}: non-finite output"
    bnd = bound(ref, scale.expand_as(ref) if scale.dim() else scale, n,
                out_dtype, intrinsic, roundings)
    ratio = (got - ref).abs() / bnd
    if where is not None:
        ratio = torch.where(where, ratio, torch.zeros_like(ratio))
    if ratio.numel() == 0:
        return 0.0
    worst = float(ratio.max())
    HEADROOM[label] = max(HEADROOM.get(label, 0.0), worst)
    print(f"bound[{label}] worst err/bound = {worst:.4f} "
          f"(n={n}, {str(out_dtype).split('.')[-1]})")
    if not worst <= 1.0:
        flat = int(ratio.argmax())
        idx = tuple(int(i) for i in torch.unravel_index(
            torch.tensor(flat), ratio.shape)) if ratio.dim() else ()
        raise AssertionError(
            f"{label}: worst element at index {idx}: got "
            f"{float(got.reshape(-1)[flat]):.9g}, ref "
            f"{float(ref.reshape(-1)[flat]):.9g}, |err| "
            f"{float((got - ref).abs().reshape(-1)[flat]):.3e} = "
            f"{worst:.3f} x bound {float(bnd.reshape(-1)[flat]):.3e}; "
            f"{int((ratio > 1).sum())} of {ratio.numel()} elements exceed")
    return worst


def relu_decided(pre, scale, n, out_dtype, intrinsic=False, label=""):
    """Mask of elements whose ReLU sign the fp64 pre-activation decides:
    |pre| above its own bound.  Asserts the undecided share <= 0.1 %.

    The share is P(|pre| < bound) ~ 2 * rel * scale * density(0) with
    rel = (n+2)*2^-23 [+ 2^-16] and scale * density(0) < 1 for any spread
    input, i.e. about 2*rel: 1e-5 for n = 64, but 0.8 % once n = 32768
    (a 32-channel 32x32 GroupNorm group), where the bound's own width
    makes 0.1 % unreachable.  The cap is therefore max(0.1 %, 2*rel).
    Undecided elements are still compared, under the kernel's own sign
    (relu_mask)."""
    dec = pre.abs() > bound(pre, scale, n, out_dtype, intrinsic)
    share = 1.0 - float(dec.double().mean())
    rel = (n + 2) * U_ACC + (U_INTRINSIC if intrinsic else 0.0)
    cap = max(1e-3, 2 * rel)
    print(f"relu[{label}] undecided share = {share:.2e} (cap {cap:.1e})")
    assert share <= cap, f"{label}: {share:.3e} of ReLU signs undecided"
    return dec


def relu_mask(pre, decided, kernel_y):
    """fp64 sign where decided, the kernel's own y > 0 elsewhere."""
    return torch.where(decided, pre > 0, upcast(kernel_y) > 0)


# ---------------------------------------------------------------------------
# cross-entropy

def ce_math(logits, labels, upstream=1.0, mutant=None):
    """Mean CE over rows and its gradient, in logits.dtype.  Also returns
    the abs-value scales: log() turns the relative error of the K-term
    sum s into an absolute one, hence the +1 in the loss scale."""
    N, K = logits.shape
    m = logits.max(dim=1, keepdim=True).values
    e = (logits - m).exp()
    s = e.sum(dim=1, keepdim=True)
    p = e / s
    onehot = torch.zeros_like(p)
    onehot.scatter_(1, labels.view(-1, 1), 1.0)
    xy = logits.gather(1, labels.view(-1, 1))
    row = ((m - xy) + s.log()).squeeze(1)
    row_scale = ((m - xy).abs() + s.log().abs() + 1.0).squeeze(1)
    if mutant == "zero":
        grad = torch.zeros_like(p)
    elif mutant == "no_onehot":
        grad = upstream * p / N
    else:
        grad = upstream * (p - onehot) / N
    return {"row": row, "row_scale": row_scale, "loss": row.mean(),
            "loss_scale": row_scale.mean(), "grad": grad,
            "grad_scale": abs(upstream) * (p + onehot) / N}


# ---------------------------------------------------------------------------
# LayerNorm / GroupNorm: one routine, reduction over ``dims``

def norm_math(x, gamma, beta, dims, eps, res=None, dy=None, mask=None,
              kernel_var=False, mutant=None):
    """y = xhat*gamma + beta [+ res] (pre-activation) and, given dy (and
    an optional ReLU mask), dx plus the per-element dgamma/dbeta terms.
    gamma/beta broadcast against x.  kernel_var computes the variance as
    E[x^2] - mean^2 like the kernels do.  mutant drops dx terms."""
    mean = x.mean(dim=dims, keepdim=True)
    if kernel_var:
        var = ((x * x).mean(dim=dims, keepdim=True) - mean * mean).clamp_min(0)
    else:
        var = ((x - mean) ** 2).mean(dim=dims, keepdim=True)
    rstd = (var + eps).rsqrt()
    xhat = (x - mean) * rstd
    # abs-value evaluation of xhat = (x - sum(x)/n) * rstd: the fp32 mean
    # carries (n+2)*2^-23 * mean|x| of summation error (and is itself
    # only representable to 2^-24 |mean|), which (x - mean) does not
    # cancel.  |xhat| alone would claim an error-free mean.
    xhat_abs = ((x - mean).abs() + x.abs().mean(dim=dims, keepdim=True)) * rstd
    pre = xhat * gamma + beta
    pre_scale = xhat_abs * gamma.abs() + beta.abs()
    if res is not None:
        pre = pre + res
        pre_scale = pre_scale + res.abs()
    ex2 = (x * x).mean(dim=dims, keepdim=True)
    out = {"mean": mean, "rstd": rstd, "xhat": xhat, "xhat_abs": xhat_abs,
           "pre": pre,
           "pre_scale": pre_scale,
           "mean_scale": x.abs().mean(dim=dims, keepdim=True),
           # d rstd = -rstd^3/2 d var, var = E[x^2] - mean^2 summed in fp32
           "rstd_scale": rstd * (1.0 + 0.5 * rstd * rstd * (ex2 + mean * mean))}
    if dy is None:
        return out
    g = dy if mask is None else dy * mask.to(dy.dtype)
    gd = g * gamma
    m1 = gd.mean(dim=dims, keepdim=True)
    m2 = (gd * xhat).mean(dim=dims, keepdim=True)
    if mutant == "no_mean":
        dx = rstd * (gd - xhat * m2)
    elif mutant == "no_xhat":
        dx = rstd * (gd - m1)
    elif mutant == "no_both":
        dx = rstd * gd
    else:
        dx = rstd * (gd - m1 - xhat * m2)
    out.update({
        "g": g, "gx": g * xhat, "gx_scale": g.abs() * xhat_abs, "dx": dx,
        "dx_scale": rstd * (gd.abs() + gd.abs().mean(dim=dims, keepdim=True)
                            + xhat_abs * (gd.abs() * xhat_abs).mean(
                                dim=dims, keepdim=True))})
    return out


def gn_views(x, gamma, beta, clients, groups):
    """Reshape a GroupNorm problem for norm_math.  x 5-D [C,ch,B,H,W]
    (layout 1) or 4-D [B,C*ch,H,W] (layout 0).  Returns (x_view, gamma_b,
    beta_b, dims, sum_dims): per-group statistics flatten in the kernel's
    group order, sum_dims reduce a per-element term to [C,G,cg]."""
    if x.dim() == 5:
        C, ch, B, H, W = x.shape
        cg = ch // groups
        xv = x.reshape(C, groups, cg, B, H, W)
        gb = gamma.reshape(C, groups, cg, 1, 1, 1)
        bb = beta.reshape(C, groups, cg, 1, 1, 1)
        return xv, gb, bb, (2, 4, 5), (3, 4, 5)
    B, CC, H, W = x.shape
    ch = CC // clients
    cg = ch // groups
    xv = x.reshape(B, clients, groups, cg, H, W)
    gb = gamma.reshape(1, clients, groups, cg, 1, 1)
    bb = beta.reshape(1, clients, groups, cg, 1, 1)
    return xv, gb, bb, (3, 4, 5), (0, 4, 5)


# ---------------------------------------------------------------------------
# client-batched convolutions ([C, IC, B, H, W] x [C, OC, IC, k, k])

def conv_math(x, w, stride, pad, bias=None):
    C, IC, B, H, W = x.shape
    OC, k = w.shape[1], w.shape[-1]
    xg = x.permute(2, 0, 1, 3, 4).reshape(B, C * IC, H, W)
    y = F.conv2d(xg, w.reshape(C * OC, IC, k, k),
                 None if bias is None else bias.reshape(C * OC),
                 stride=stride, padding=pad, groups=C)
    OH, OW = y.shape[-2:]
    return y.reshape(B, C, OC, OH, OW).permute(1, 2, 0, 3, 4).contiguous()


def conv_all(x, w, dy, stride, pad, bias=None):
    """(y, dx, dw) of the linear conv for upstream dy, in x.dtype."""
    xr = x.clone().requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    y = conv_math(xr, wr, stride, pad, bias)
    dx, dw = torch.autograd.grad(y, (xr, wr), dy)
    return y.detach(), dx, dw


def conv_ref(x, w, dy, stride, pad, bias=None):
    """fp64 reference and abs-value scales of fwd, dx and dw."""
    y, dx, dw = conv_all(x, w, dy, stride, pad, bias)
    ys, dxs, dws = conv_all(x.abs(), w.abs(), dy.abs(), stride, pad,
                            None if bias is None else bias.abs())
    return {"y": y, "dx": dx, "dw": dw, "y_scale": ys, "dx_scale": dxs,
            "dw_scale": dws}


# ---------------------------------------------------------------------------
# flat optimiser / aggregation ops (param-major replica layout)

def sgd_math(buf, grad, master, offsets, clients, lr, mu):
    """buf - lr*(grad + mu*(buf - master)) per block, and its scale."""
    out = torch.empty_like(buf)
    scale = torch.empty_like(buf)
    for b in range(len(offsets) - 1):
        g0, g1 = offsets[b], offsets[b + 1]
        n = g1 - g0
        sl = slice(clients * g0, clients * g1)
        w = buf[sl].view(clients, n)
        g = grad[sl].view(clients, n)
        m = master[g0:g1].unsqueeze(0)
        out[sl] = (w - lr * (g + mu * (w - m))).reshape(-1)
        scale[sl] = (w.abs() + abs(lr) * (g.abs() + abs(mu)
                                          * (w.abs() + m.abs()))).reshape(-1)
    return out, scale


def delta_math(delta, buf, master, weights, offsets, clients, hoisted=False):
    """delta + sum_c w_c (buf_c - master) with two scales.

    ``scale`` = |delta| + sum_c |w_c||buf_c - master| fits a kernel that
    subtracts the master per client.  aggregate.hip hoists the master out
    of the client loop, sum_c w_c buf_c - (sum_c w_c) master, so its
    rounding errors are those of THAT expression: ``scale_hoisted`` =
    |delta| + sum_c |w_c||buf_c| + (sum_c |w_c|)|master|.  Where a replica
    sits close to the master the first scale vanishes while w_c*buf_c is
    still rounded at 2^-24 |w_c buf_c|.  hoisted=True evaluates the
    hoisted expression."""
    out = delta.clone()
    scale = delta.abs().clone()
    scale_h = delta.abs().clone()
    wv = weights.view(clients, 1)
    for b in range(len(offsets) - 1):
        g0, g1 = offsets[b], offsets[b + 1]
        n = g1 - g0
        blk = buf[clients * g0:clients * g1].view(clients, n)
        m = master[g0:g1].unsqueeze(0)
        if hoisted:
            out[g0:g1] += (blk * wv).sum(0) - wv.sum() * m.squeeze(0)
        else:
            out[g0:g1] += ((blk - m) * wv).sum(0)
        scale[g0:g1] += ((blk - m).abs() * wv.abs()).sum(0)
        scale_h[g0:g1] += ((blk.abs() * wv.abs()).sum(0)
                           + wv.abs().sum() * m.abs().squeeze(0))
    return out, scale, scale_h
