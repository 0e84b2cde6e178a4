"""fp64 single-step references of the fused LSTM kernels (ops/csrc/lstm.hip)
and the bounds test_lstm_fused_gpu.py holds them to.

Both directions are teacher-forced on what the kernel itself stored, which
turns an L-step recurrence into L single operations with one-step bounds:

forward, step t, from the kernel's own hs[t-1] (bf16, exactly what its
MFMAs read) and cs[t-1] (fp32, exactly what it carried):
  pre = xp_t + h_{t-1} W: the accumulator is seeded with xp exactly and
  sums H products in fp32, |d pre| <= (H+2) 2^-23 (|xp| + |h||W|).  Every
  activation is 1-Lipschitz and bounded by 1, and is built from a fast
  exp2 and a reciprocal: e_gate = ((H+2) 2^-23 + 2^-16) (|xp| + |h||W| + 1)
  before the one bf16 rounding of the stored gate.
  c_t = f c_{t-1} + i g from the fp32 gates: two terms in fp32, plus
  e_f |c| + e_i |g| + e_g |i| + e_i e_g inherited.
  h_t = o tanh(c_t): one bf16 rounding, the fast tanh, plus e_o and |o|
  times the whole error of c_t inherited.

backward, step t, from the kernel's own stored bf16 dgates_{t+1}:
  dh_t = dhs_t + dgates_{t+1} W^T (4H products in fp32); dc is carried in
  fp32 over L-1-t steps of an fma and a product each, and the pointwise
  formulas are six more products: n = 4H + 4 (L-t) + 6 fp32 operations over
  the absolute-value chain (|dhs| + |dgates||W|^T, and 1 - x^2 -> 1 + x^2,
  i (1-i) -> i (1+i)), one fast tanh, one bf16 rounding.
"""

import torch

import kernel_bounds as kb

BF16, F32 = torch.bfloat16, torch.float32


def _shift(x):
    """x[:, :, t-1] at t, zeros at t = 0."""
    return torch.cat([torch.zeros_like(x[:, :, :1]), x[:, :, :-1]], dim=2)


def _acts(pre, H):
    i, f, g, o = pre.split(H, dim=-1)
    return torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)


def check_forward(xp, w, hs, gates, cs, label):
    H = w.shape[1]
    xp, w, hs_k, gates_k, cs_k = (kb.upcast(t) for t in (xp, w, hs, gates, cs))
    h_prev, c_prev = _shift(hs_k), _shift(cs_k)
    pre = xp + torch.einsum("cblh,chn->cbln", h_prev, w)
    pre_scale = xp.abs() + torch.einsum("cblh,chn->cbln", h_prev.abs(), w.abs())
    i, f, g, o = _acts(pre, H)
    kb.assert_bounded(gates_k, torch.cat([i, f, g, o], -1), pre_scale + 1.0, H,
                      BF16, intrinsic=True, label=label + ".gates")
    e = ((H + 2) * kb.U_ACC + kb.U_INTRINSIC) * (pre_scale + 1.0)
    e_i, e_f, e_g, e_o = e.split(H, dim=-1)
    c = f * c_prev + i * g
    c_scale = f * c_prev.abs() + i * g.abs()
    c_extra = e_f * c_prev.abs() + e_i * g.abs() + e_g * i + e_i * e_g
    kb.assert_bounded(cs_k, c, c_scale, 2, F32, label=label + ".cs",
                      extra=c_extra)
    e_c = kb.bound(c, c_scale, 2, F32, extra=c_extra)
    kb.assert_bounded(hs_k, o * torch.tanh(c), o, 1, BF16, intrinsic=True,
                      label=label + ".hs", extra=e_o + o * e_c)


def check_backward(dhs, gates, cs, hs, w, dgates, dw, label):
    C, B, L, H = hs.shape
    dhs, gates, cs, hs, w, dg_k = (kb.upcast(t)
                                   for t in (dhs, gates, cs, hs, w, dgates))
    i, f, g, o = gates.split(H, dim=-1)
    c_prev, tc = _shift(cs), torch.tanh(cs)
    dc = dc_abs = torch.zeros(C, B, H, dtype=torch.float64)
    for t in range(L - 1, -1, -1):
        dh, dh_abs = dhs[:, :, t], dhs[:, :, t].abs()
        if t + 1 < L:
            nxt = dg_k[:, :, t + 1]
            dh = dh + torch.einsum("cbn,chn->cbh", nxt, w)
            dh_abs = dh_abs + torch.einsum("cbn,chn->cbh", nxt.abs(), w.abs())
        it, ft, gt, ot = (x[:, :, t] for x in (i, f, g, o))
        tct, cpt = tc[:, :, t], c_prev[:, :, t]
        dc = dc + dh * ot * (1 - tct * tct)
        dc_abs = dc_abs + dh_abs * ot * (1 + tct * tct)
        ref = torch.cat([dc * gt * it * (1 - it), dc * cpt * ft * (1 - ft),
                         dc * it * (1 - gt * gt), dh * tct * ot * (1 - ot)], -1)
        scale = torch.cat([dc_abs * gt.abs() * it * (1 + it),
                           dc_abs * cpt.abs() * ft * (1 + ft),
                           dc_abs * it * (1 + gt * gt),
                           dh_abs * tct.abs() * ot * (1 + ot)], -1)
        kb.assert_bounded(dg_k[:, :, t], ref, scale, 4 * H + 4 * (L - t) + 6,
                          BF16, intrinsic=True, label=f"{label}.dgates.t{t}")
        dc, dc_abs = dc * ft, dc_abs * ft
    h_prev = _shift(hs).reshape(C, B * L, H)
    dg2 = dg_k.reshape(C, B * L, 4 * H)
    kb.assert_bounded(dw, torch.bmm(h_prev.transpose(1, 2), dg2),
                      torch.bmm(h_prev.abs().transpose(1, 2), dg2.abs()),
                      B * L, BF16, label=label + ".dw")
