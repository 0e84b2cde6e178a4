"""Derived element-wise error bounds for kernel-vs-fp64 comparisons.

Every numerics test of a HIP kernel compares the kernel output with an
fp64 reference computed from ``upcast`` copies of the exact tensors the
kernel received, and accepts

    |got - ref| <= roundings*u_out*|ref| + (n+2)*2^-23*scale
                   + intrinsic*2^-16*scale + 2^-126

- ``u_out``: 2^-8 for a bf16 output: bf16 carries 8 significant bits, so
  2^-8 is exactly ONE round-to-nearest (a lone rounding is observed at up
  to 0.996 of it).  2^-11 likewise for fp16 (11 significant bits).
  2^-22 for an fp32 output (4 roundings).  A result
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
  returned as 0.  An fp16 output has 2^-25 in its place: half the
  spacing of the fp16 denormals, which the hardware keeps.

An operation whose input was itself computed inexactly (the second
rounding of bmm + bias, the tied head's rounded logits) adds the
propagated error as an absolute ``extra`` term, derived at the call.

These numbers are derived, not fitted: a kernel that exceeds them is a
finding.  The module also holds the dtype-generic math of the checked
operations, run in fp64 as the reference and (by the CPU tests) in fp32
as a stand-in kernel that the bound must accept and whose mutants it
must reject.
"""

from __future__ import annotations

import torch
import torch.nn.functional as F

U_OUT = {torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -22,
         torch.float16: 2.0 ** -11}
U_ACC = 2.0 ** -23
U_INTRINSIC = 2.0 ** -16
FTZ_FLOOR = 2.0 ** -126
# fp16 has 5 exponent bits: below 2^-14 its values are spaced 2^-24 apart
# (gfx9 keeps fp16 denormals), so one rounding there is absolute
FLOOR = {torch.float16: 2.0 ** -25}

# worst err/bound ratio seen per label in this process (information only)
HEADROOM: dict = {}


def upcast(t: torch.Tensor) -> torch.Tensor:
    """fp64 CPU copy of the exact tensor a kernel received."""
    return t.detach().to(device="cpu", dtype=torch.float64)


def bound(ref, scale, n, out_dtype, intrinsic=False, roundings=1, extra=0.0):
    """``extra`` is an absolute allowance (scalar or tensor like ref) for
    error the operation inherits from an input that was itself computed
    inexactly; the caller derives it.  0 leaves the bound as documented."""
    rel = (n + 2) * U_ACC + (U_INTRINSIC if intrinsic else 0.0)
    return (roundings * U_OUT[out_dtype] * ref.abs() + rel * scale
            + FLOOR.get(out_dtype, FTZ_FLOOR) + extra)


def assert_bounded(got, ref, scale, n, out_dtype, intrinsic=False,
                   where=None, label="", roundings=1, extra=0.0):
    """Assert |got - ref| <= bound element-wise (optionally only ``where``).
    Returns the worst error as a fraction of its bound."""
    got = upcast(got)
    ref = ref.to(torch.float64)
    scale = torch.as_tensor(scale, dtype=torch.float64)
    assert got.shape == ref.shape, (label, tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all()), f"{label}: non-finite output"
    bnd = bound(ref, scale.expand_as(ref) if scale.dim() else scale, n,
                out_dtype, intrinsic, roundings, extra)
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


# ---------------------------------------------------------------------------
# per-client linear (models/base.py _BLinearFn)

def linear_math(x, w, b, dy, mutant=None):
    """y = x @ w [+ b] and the gradients for upstream dy, in x.dtype:
    x [C, rows, in], w [C, in, out], b [C, out] or None, dy [C, rows, out].
    Returns y, dx, dw, db, the bias-free product xw, and the abs-value
    scale of each.  Mutants: dw from the untransposed operand (x's memory
    reinterpreted as [C, in, rows]), db dropped, dx off by 1 %."""
    C, rows, fin = x.shape
    xw = torch.bmm(x, w)
    xw_scale = torch.bmm(x.abs(), w.abs())
    y, y_scale = xw, xw_scale
    if b is not None:
        y = xw + b.unsqueeze(1)
        y_scale = xw_scale + b.abs().unsqueeze(1)
    dx = torch.bmm(dy, w.transpose(1, 2))
    if mutant == "dx_1pct":
        dx = dx * 1.01
    xt = x.transpose(1, 2)
    if mutant == "dw_untransposed":
        xt = x.contiguous().view(C, fin, rows)
    dw = torch.bmm(xt, dy)
    db = dy.sum(dim=1)
    if mutant == "db_dropped":
        db = torch.zeros_like(db)
    return {"y": y, "y_scale": y_scale, "xw": xw, "xw_scale": xw_scale,
            "dx": dx, "dx_scale": torch.bmm(dy.abs(), w.abs().transpose(1, 2)),
            "dw": dw, "dw_scale": torch.bmm(x.abs().transpose(1, 2), dy.abs()),
            "db": db, "db_scale": dy.abs().sum(dim=1)}


def assert_linear_bounded(got, ref, dtype, has_bias, label="blinear"):
    """got: dict y/dx/dw[/db] of a per-client linear; ref: linear_math in
    fp64 on upcast operands.  Reduction lengths: y in, dx out, dw rows,
    db rows.

    With a bias the forward is ``bmm`` (stored in ``dtype``: error
    e1 <= u|xw| + (in+2) 2^-23 |x||w|) followed by an add that is rounded
    again, relative to the sum it formed: u|xw + e1 + b| <= u|y| + u|e1|.
    Total: u|y| + (in+2) 2^-23 |x||w| + u|xw| + u|e1|.  The first two are
    the ordinary bound of y; the rest is passed as ``extra``.  It is
    relative to |xw|, not |y|: xw and b can cancel, so ``roundings=2``
    (2u|y|) would be wrong."""
    rows, fin = ref["dx"].shape[1], ref["dx"].shape[2]
    fout = ref["y"].shape[2]
    extra = 0.0
    if has_bias:
        u = U_OUT[dtype]
        extra = u * (ref["xw"].abs()
                     + bound(ref["xw"], ref["xw_scale"], fin, dtype))
    assert_bounded(got["y"], ref["y"], ref["y_scale"], fin, dtype,
                   label=label + ".y", extra=extra)
    assert_bounded(got["dx"], ref["dx"], ref["dx_scale"], fout, dtype,
                   label=label + ".dx")
    assert_bounded(got["dw"], ref["dw"], ref["dw_scale"], rows, dtype,
                   label=label + ".dw")
    if has_bias:
        assert_bounded(got["db"], ref["db"], ref["db_scale"], rows, dtype,
                       label=label + ".db")


# ---------------------------------------------------------------------------
# tied LM head + cross-entropy (models/bert.py _TiedHeadCE)

def tied_head_math(hs, tok, bias, labels, slice_v):
    """Full-logits form of mean_n CE(hs @ tok^T + bias, labels) in
    hs.dtype: hs [C, N, H], tok [C, V, H], bias [C, V], labels [C, N].
    Returns loss, dhs, dtok, dbias for upstream 1 and the intermediate
    and abs-value quantities the bound needs.  ``slice_v`` only groups
    the abs-value partial sums of dhs the way the sliced code forms
    them; the values do not depend on it."""
    C, N, H = hs.shape
    V = tok.shape[1]
    g = 1.0 / (C * N)
    z0 = torch.bmm(hs, tok.transpose(1, 2))              # [C, N, V]
    z = z0 + bias.unsqueeze(1)
    z_scale = torch.bmm(hs.abs(), tok.abs().transpose(1, 2)) \
        + bias.abs().unsqueeze(1)
    ce = ce_math(z.reshape(C * N, V), labels.reshape(C * N))
    p = (z - z.logsumexp(dim=2, keepdim=True)).exp()
    onehot = torch.zeros_like(p)
    onehot.scatter_(2, labels.unsqueeze(2), 1.0)
    dl = g * (p - onehot)
    dl_scale = g * (p + onehot)
    part_abs = torch.zeros_like(hs)
    for s0 in range(0, V, slice_v):
        s1 = min(s0 + slice_v, V)
        part_abs = part_abs + torch.bmm(dl[:, :, s0:s1], tok[:, s0:s1]).abs()
    return {"loss": ce["loss"], "loss_scale": ce["loss_scale"],
            "z0": z0, "z_scale": z_scale, "p": p, "dl": dl,
            "dl_scale": dl_scale, "g": g,
            "dhs": torch.bmm(dl, tok), "dhs_scale": torch.bmm(dl_scale, tok.abs()),
            "dhs_part_abs": part_abs,
            "dtok": torch.bmm(dl.transpose(1, 2), hs),
            "dtok_scale": torch.bmm(dl_scale.transpose(1, 2), hs.abs()),
            "dbias": dl.sum(dim=1), "dbias_scale": dl_scale.sum(dim=1)}


def assert_tied_head_bounded(got, ref, hs, tok, dtype, slice_v, label="tied"):
    """got: dict loss/dhs/dtok/dbias of the sliced tied head; ref:
    tied_head_math in fp64 on upcast operands (hs, tok also upcast).

    Rounding points of _TiedHeadCE, in order:

    1. Each logit is a bmm output stored in ``dtype`` before ``.float()``
       and the fp32 bias add: |dz| <= d_z = bound(hs.tok, |hs||tok| +
       |bias|, H+1, dtype).  d = max_j d_z per row.
    2. lse is 1-Lipschitz in the max norm and z_y moves by at most d, so
       a row loss moves by at most 2d, plus its fp32 evaluation over V
       terms; the mean over C*N rows is one more fp32 sum.  torch.exp /
       torch.log are correctly rounded library calls, not fast
       intrinsics: no intrinsic term.
    3. p_j = exp(z_j - lse): both move by at most d, so |dp_j| <=
       p_j (e^{2d} - 1).  dlogits = g (p - onehot) is evaluated in fp32
       (length-V term on g (p + onehot)) and stored in ``dtype``: one
       rounding, of the perturbed value.  E_dl is the sum of the three.
    4. dbias and dtok sum N perturbed dlogits (times |hs| for dtok):
       the propagated sum of E_dl, the fp32 sum (N+2) 2^-23 scale, one
       output rounding.
    5. dhs = sum over S slices of a GEMM whose output is stored in
       ``dtype`` (one rounding per partial), accumulated by ``dhs +=``
       in ``dtype`` starting from zero (the first add is exact, the other
       S-1 round once each).  Every rounded quantity is at most
       (1+u)^(2S-1) sum_s |partial_s|, so: (2S-1) u (1+u)^(2S-1)
       sum_s |partial_s|, plus the propagated sum of E_dl |tok| and the
       fp32 sum over V.  The output rounding is one of those (2S-1)."""
    C, N, H = hs.shape
    V = tok.shape[1]
    S = (V + slice_v - 1) // slice_v
    u = U_OUT[dtype]
    g = ref["g"]
    d_z = bound(ref["z0"], ref["z_scale"], H + 1, dtype)
    d = d_z.max(dim=2, keepdim=True).values                     # [C, N, 1]
    assert_bounded(got["loss"], ref["loss"], ref["loss_scale"], V + C * N,
                   torch.float32, label=label + ".loss",
                   extra=float((2 * d).mean()))
    dp = g * ref["p"] * torch.expm1(2 * d)
    e_dl = bound(ref["dl"], ref["dl_scale"], V, dtype) + (1 + u) * dp
    assert_bounded(got["dbias"], ref["dbias"], ref["dbias_scale"], N, dtype,
                   label=label + ".dbias", extra=e_dl.sum(dim=1))
    assert_bounded(got["dtok"], ref["dtok"], ref["dtok_scale"], N, dtype,
                   label=label + ".dtok",
                   extra=torch.bmm(e_dl.transpose(1, 2), hs.abs()))
    assert_bounded(got["dhs"], ref["dhs"], ref["dhs_scale"], V, dtype,
                   label=label + ".dhs", roundings=0,
                   extra=((2 * S - 1) * u * (1 + u) ** (2 * S - 1)
                          * ref["dhs_part_abs"]
                          + torch.bmm(e_dl, tok.abs())))


# ---------------------------------------------------------------------------
# model-level gradients: device fp32 against the same model in fp64

MODEL_CASES = {
    # name -> (constructor kwargs, clients, batch, k): k = fast-intrinsic
    # custom-kernel calls on the GPU path - the HIP cross-entropy for MLP
    # and LSTM; BERT's tied head uses no fast intrinsic but each of its
    # 1 + 2*layers LayerNorms does.
    "mlp": (dict(in_features=40, hidden=24, num_classes=10), 3, 8, 1),
    "lstm": (dict(vocab_size=30, embed=8, hidden=16, layers=2, seq_len=4),
             3, 8, 1),
    "bert": (dict(seq_len=8, vocab_size=40, hidden=32, layers=2, heads=2),
             3, 4, 5),
}
_MODEL_CACHE: dict = {}


def _rel_max(g, g64):
    return float((g.detach().double().cpu() - g64).abs().max()
                 / g64.abs().max())


def model_loss_and_grads(model, params, x, y):
    """model.loss and its gradient per parameter tensor."""
    leaves = {k: v.detach().clone().requires_grad_(True)
              for k, v in params.items()}
    loss = model.loss(leaves, x, y)
    grads = torch.autograd.grad(loss, list(leaves.values()))
    return loss.detach(), dict(zip(leaves, grads))


def model_case(name):
    """Model, per-client perturbed fp32 parameters (the values every path
    receives), inputs, the fp64 reference and e_cpu32; built once.

    The fp64 reference runs the model's CPU forward on fp64 copies and
    takes the cross-entropy through ce_math in fp64 (the CPU
    cross_entropy_fwd_bwd casts its logits to fp32).  e_cpu32 is the
    worst max|g - g64| / max|g64| over the loss and all parameter
    gradients of the CPU fp32 composed path."""
    if name in _MODEL_CACHE:
        return _MODEL_CACHE[name]
    from olearning_sim_amd.models import build_model
    kwargs, C, B, k = MODEL_CASES[name]
    model = build_model(name, **kwargs)
    gen = torch.Generator().manual_seed(17)
    gp = model.init_global(generator=gen)
    params = {}
    for key, v in gp.items():
        rep = v.float().unsqueeze(0).expand(C, *v.shape).clone()
        params[key] = rep + 0.01 * torch.randn(rep.shape, generator=gen)
    if model.sequence_model:
        V, L = model.vocab_size, model.seq_len
        x = torch.randint(0, V, (C, B, L), generator=gen)
        y = torch.randint(0, V, (C, B, L), generator=gen)
    else:
        x = torch.randn((C, B) + tuple(model.input_shape), generator=gen)
        y = torch.randint(0, model.num_classes, (C, B), generator=gen)

    p64 = {key: v.double().requires_grad_(True) for key, v in params.items()}
    logits = model.forward(p64, x if model.sequence_model else x.double())
    K = logits.shape[-1]
    loss64 = ce_math(logits.reshape(-1, K), y.reshape(-1))["loss"]
    g64 = dict(zip(p64, torch.autograd.grad(loss64, list(p64.values()))))
    loss64 = loss64.detach()
    for key, g in g64.items():
        assert float(g.abs().max()) > 0, f"{name}: {key} has a zero gradient"

    loss32, g32 = model_loss_and_grads(model, params, x, y)
    e_cpu32 = max([abs(float(loss32) - float(loss64)) / abs(float(loss64))]
                  + [_rel_max(g32[key], g64[key]) for key in g64])
    case = {"model": model, "params": params, "x": x, "y": y, "k": k,
            "loss64": loss64, "g64": g64, "e_cpu32": e_cpu32}
    _MODEL_CACHE[name] = case
    return case


def assert_model_bounded(name, loss, grads):
    """Loss and every parameter gradient within
    tol = 64 * k * max(e_cpu32, 2^-22) of fp64, relative to the largest
    reference element of the tensor.

    e_cpu32 is what the plain fp32 composition of the same model loses
    against fp64 (floored at one fp32 output unit); a HIP kernel may use
    fast intrinsics, whose unit U_INTRINSIC is 64 x U_OUT[float32], and k
    such kernels sit on the path.  Nothing here is read off the code
    under test.  Returns the worst e / tol."""
    case = model_case(name)
    tol = (U_INTRINSIC / U_OUT[torch.float32]) * case["k"] \
        * max(case["e_cpu32"], U_OUT[torch.float32])
    errs = {"loss": abs(float(loss) - float(case["loss64"]))
            / abs(float(case["loss64"]))}
    for key, g64 in case["g64"].items():
        assert bool(torch.isfinite(grads[key]).all()), f"{name}: {key}"
        errs[key] = _rel_max(grads[key], g64)
    worst = max(errs, key=errs.get)
    ratio = errs[worst] / tol
    HEADROOM["model." + name] = max(HEADROOM.get("model." + name, 0.0), ratio)
    print(f"model[{name}] e_cpu32 = {case['e_cpu32']:.2e}, tol = {tol:.2e}, "
          f"worst e/tol = {ratio:.4f} ({worst})")
    bad = {key: f"{e / tol:.1f}x" for key, e in errs.items() if not e <= tol}
    assert not bad, f"{name}: beyond tol {tol:.2e}: {bad}"
    return ratio


# ---------------------------------------------------------------------------
# the local trainer's chunk: device fp32 against a per-client fp64 reference

def _f32(v):
    """The value a launcher receives when handed the Python float v."""
    return float(torch.tensor(float(v), dtype=torch.float32))


def _trainer_locals(model, global_params, batches, lr, mu, steps):
    """Each client's fp64 parameters after ``steps`` local SGD / FedProx
    steps from the global parameters, one client at a time (C = 1)."""
    g64 = {k: v.detach().double().cpu() for k, v in global_params.items()}
    clients = batches[0][1].shape[0]
    lr, mu = _f32(lr), _f32(mu)
    finals = []
    for c in range(clients):
        p = {k: v.clone().unsqueeze(0) for k, v in g64.items()}
        for step in range(steps):
            x, y = batches[step]
            xc, yc = x[c:c + 1], y[c:c + 1]
            if xc.is_floating_point():
                xc = xc.double()
            leaves = {k: v.requires_grad_(True) for k, v in p.items()}
            logits = model.forward(leaves, xc)
            K = logits.shape[-1]
            loss = ce_math(logits.reshape(-1, K), yc.reshape(-1))["loss"]
            grads = torch.autograd.grad(loss, list(leaves.values()),
                                        allow_unused=True)
            p = {}
            for (k, w), g in zip(leaves.items(), grads):
                w = w.detach()
                if g is None:
                    g = torch.zeros_like(w)
                p[k] = w - lr * (g + mu * (w - g64[k].unsqueeze(0)))
        finals.append({k: v.squeeze(0) for k, v in p.items()})
    return g64, finals


def _trainer_aggregate(g64, finals, weights, clip_norm):
    w = torch.as_tensor(weights, dtype=torch.float64)
    sq = torch.stack([sum(((p[k] - g64[k]) ** 2).sum() for k in g64)
                      for p in finals])
    s = torch.ones_like(sq)
    if clip_norm > 0.0:
        S = _f32(clip_norm)
        s = torch.where(sq > S * S, S / sq.sqrt(), s)
    w_eff = w * s
    delta = {k: sum(w_eff[c] * (p[k] - g64[k]) for c, p in enumerate(finals))
             for k in g64}
    return delta, sq, w_eff


def trainer_math(model, global_params, batches, weights, lr, mu, steps,
                 clip_norm):
    """What one training round of a set of clients adds to the delta
    accumulator, in fp64 and with none of the trainer's code.

    batches[step] = (x [C, B, ...], y [C, B]).  Client c on its own: start
    from the global parameters; per step, model.forward on its slice of
    the batch (C = 1), the loss the mean over ITS rows (ce_math), then
    p -= lr * (g + mu * (p - p_global)).  Then
    sq[c] = sum ||p_c - p_global||^2, s_c = S / sqrt(sq[c]) where
    sq[c] > S^2 else 1 (clip_norm = 0: no clipping), and
    delta[k] = sum_c w_c s_c (p_c[k] - p_global[k]).  lr, mu and S at
    their fp32 values.  Returns (delta per parameter, sq [C], the
    effective weights w_c s_c [C])."""
    g64, finals = _trainer_locals(model, global_params, batches, lr, mu,
                                  steps)
    return _trainer_aggregate(g64, finals, weights, clip_norm)


class FixedData:
    """Stand-in for the trainer's ``data``: pre-drawn CPU batches, the
    same numbers on every device (SyntheticFederatedData draws from a
    device generator).  batches[step] = (x [N, B, ...], y [N, B]) over all
    N clients; batch() returns the rows of client_ids on ``device``,
    floating-point inputs in the requested dtype."""

    def __init__(self, batches, device="cpu"):
        self.batches = batches
        self.device = torch.device(device)

    def batch(self, client_ids, round_idx, step, batch_size, dtype):
        x, y = self.batches[step]
        ids = client_ids.cpu()
        assert x.shape[1] == batch_size
        xs = x[ids].to(self.device)
        if xs.is_floating_point():
            xs = xs.to(dtype)
        return xs, y[ids].to(self.device)


# Updates must stand clear of the fp32 spacing of the weights, or e_cpu32
# is storage rounding alone (LSTM: 2.6e-3 at lr 0.05, 1.4e-4 at lr 1.0).
TRAINER_LR = {"mlp": 0.3, "lstm": 1.0, "bert": 0.3}
TRAINER_STEPS = 3
TRAINER_MU = 0.5
TRAINER_WEIGHTS = (1.5, 0.0, 0.75)
TRAINER_CLIPS = ("off", "all", "one")
_TRAINER_CACHE: dict = {}


def _trainer_setup(name):
    """Model, global parameters, batches and the fp64 reference of every
    clip setting; built once."""
    key = "setup." + name
    if key in _TRAINER_CACHE:
        return _TRAINER_CACHE[key]
    from olearning_sim_amd.models import build_model
    kwargs, C, B, k = MODEL_CASES[name]
    assert C == len(TRAINER_WEIGHTS)
    model = build_model(name, **kwargs)
    # seed: one at which the fp64 norms of clients 0 and 2 lie more than
    # 2 % from their midpoint in all three models (asserted below at 1 %;
    # a property of the reference alone)
    gen = torch.Generator().manual_seed(53)
    gp = {key_: v.float() + 0.01 * torch.randn(v.shape, generator=gen)
          for key_, v in model.init_global(generator=gen).items()}
    batches = []
    for _ in range(TRAINER_STEPS):
        if model.sequence_model:
            V, L = model.vocab_size, model.seq_len
            x = torch.randint(0, V, (C, B, L), generator=gen)
            y = torch.randint(0, V, (C, B, L), generator=gen)
        else:
            x = torch.randn((C, B) + tuple(model.input_shape), generator=gen)
            y = torch.randint(0, model.num_classes, (C, B), generator=gen)
        batches.append((x, y))
    lr = TRAINER_LR[name]
    g64, finals = _trainer_locals(model, gp, batches, lr, TRAINER_MU,
                                  TRAINER_STEPS)
    norms = _trainer_aggregate(g64, finals, TRAINER_WEIGHTS, 0.0)[1].sqrt()
    # "all": every client clipped, each by its own factor; "one": exactly
    # one of the two weighted clients clipped
    S = {"off": 0.0, "all": _f32(0.5 * float(norms.min())),
         "one": _f32(0.5 * float(norms[0] + norms[2]))}
    ref = {}
    for clip in TRAINER_CLIPS:
        delta, sq, w_eff = _trainer_aggregate(g64, finals, TRAINER_WEIGHTS,
                                              S[clip])
        for key_, d in delta.items():
            assert float(d.abs().max()) > 0, f"{name}: {key_} does not move"
        if clip != "off":
            # fp32 must not be able to flip a clip decision
            gap = ((sq.sqrt() - S[clip]).abs() / S[clip]).min()
            assert float(gap) > 0.01, (name, clip, sq.sqrt().tolist(), S[clip])
        ref[clip] = {"delta": delta, "sq": sq, "w_eff": w_eff, "S": S[clip]}
    assert int((ref["all"]["w_eff"] < torch.tensor(TRAINER_WEIGHTS)).sum()) == 2
    clipped = ref["one"]["sq"] > ref["one"]["S"] ** 2
    assert int(clipped[0]) + int(clipped[2]) == 1
    setup = {"model": model, "gp": gp, "g64": g64, "batches": batches,
             "lr": lr, "C": C, "B": B, "k": k, "ref": ref}
    _TRAINER_CACHE[key] = setup
    return setup


def trainer_run(name, clip, device="cpu", chunks=((0, 1, 2),)):
    """LocalTrainer in fp32 on ``device`` over the case's clients, one
    train_chunk per entry of ``chunks``, all into one delta accumulator
    (each chunk clips its own clients, as the round loop does).  Returns
    (named delta views, sq [C] in client order)."""
    from olearning_sim_amd.engine.client_manager import FlatParams
    from olearning_sim_amd.engine.local_train import LocalTrainer
    su = _trainer_setup(name)
    master = FlatParams({k: v.to(device) for k, v in su["gp"].items()})
    trainer = LocalTrainer(
        su["model"], master, FixedData(su["batches"], device), lr=su["lr"],
        prox_mu=TRAINER_MU, local_steps=TRAINER_STEPS, batch_size=su["B"],
        dtype=torch.float32, clip_norm=su["ref"][clip]["S"],
        update_norm_stats=True)
    trainer.begin_round()
    delta_flat = master.zeros_like_flat()
    weights = torch.tensor(TRAINER_WEIGHTS, dtype=torch.float32)
    sq = torch.zeros(su["C"], dtype=torch.float64)
    for chunk in chunks:
        ids = torch.tensor(chunk, dtype=torch.int64)
        out = trainer.train_chunk(ids.to(device), weights[ids].to(device), 0,
                                  delta_flat)
        sq[ids] = out["sq"].detach().double().cpu()
    return master.views_of(delta_flat), sq


def _trainer_errs(ref, delta_views, sq):
    if not isinstance(delta_views, dict):
        delta_views = dict(zip(ref["delta"], delta_views))
    errs = {"sq": _rel_max(sq, ref["sq"])}
    for key, d64 in ref["delta"].items():
        assert bool(torch.isfinite(delta_views[key]).all()), key
        errs[key] = _rel_max(delta_views[key], d64)
    return errs


def trainer_case(name):
    """The setup plus e_cpu32: the worst max|got - ref| / max|ref| over
    every parameter's delta, sq and the three clip settings of the CPU
    fp32 LocalTrainer against trainer_math.  Asserts that the tolerance
    this gives, 64 * k * max(e_cpu32, 2^-22), is at most 0.05: beyond
    that, raise the learning rate, the check would separate nothing."""
    if name in _TRAINER_CACHE:
        return _TRAINER_CACHE[name]
    su = _trainer_setup(name)
    e_cpu32 = max(max(_trainer_errs(su["ref"][clip],
                                    *trainer_run(name, clip)).values())
                  for clip in TRAINER_CLIPS)
    tol = (U_INTRINSIC / U_OUT[torch.float32]) * su["k"] \
        * max(e_cpu32, U_OUT[torch.float32])
    assert tol <= 0.05, f"{name}: e_cpu32 {e_cpu32:.2e} gives tol {tol:.2e}"
    case = dict(su, e_cpu32=e_cpu32, tol=tol)
    _TRAINER_CACHE[name] = case
    return case


def assert_trainer_bounded(name, delta_views, sq, clip="off"):
    """Every parameter's accumulated delta, and sq, within
    tol = 64 * k * max(e_cpu32, 2^-22) of trainer_math, relative to the
    largest reference element of the tensor (assert_model_bounded's rule;
    nothing is read off the code under test).  delta_views: the named
    views of the accumulator, or a list in parameter order.  Returns the
    worst e / tol."""
    case = trainer_case(name)
    tol = case["tol"]
    errs = _trainer_errs(case["ref"][clip], delta_views, sq)
    worst = max(errs, key=errs.get)
    ratio = errs[worst] / tol
    label = "trainer." + name
    HEADROOM[label] = max(HEADROOM.get(label, 0.0), ratio)
    print(f"trainer[{name}.{clip}] e_cpu32 = {case['e_cpu32']:.2e}, "
          f"tol = {tol:.2e}, worst e/tol = {ratio:.4f} ({worst})")
    bad = {key: f"{e / tol:.1f}x" for key, e in errs.items() if not e <= tol}
    assert not bad, f"{name}.{clip}: beyond tol {tol:.2e}: {bad}"
    return ratio
