"""fp64 references of the fused attention kernels (ops/csrc/attn.hip) and
the bounds test_attn_fused_gpu.py holds them to.  u = 2^-8 (one bf16
rounding); every reference is computed from ``kb.upcast`` copies of what the
kernel received, for the backward including its own stored att and lse.

Rounding points of the kernels, one term each:

score     s_ij = scale * q_i . k_j: HD products accumulated in fp32 and one
          multiplication by the fp32 constant scale:
          e_s = (HD+3) 2^-23 scale |q_i|.|k_j|.
prob      p = exp2((s - m) log2e) / l forward, exp2((s - lse) log2e)
          backward: the exponent moves by at most 2 max_j e_s (s itself, and
          m or lse formed from the s of the row), the fast exp2 is the
          intrinsic: rho = 2 max_j e_s + 2^-16, relative.
lse       fp32 output m + log(l): l sums L terms (n = L), fast log2
          (intrinsic), and it inherits max_j e_s + 2^-16 from the scores and
          the exponentials under the sum.
att       O = (P V) / l: P rounded to bf16 as MFMA operand (u), numerator
          and denominator each off by rho, L products accumulated in fp32
          after a sum of L terms (n = 2L), fast reciprocal (intrinsic):
          extra = (u + 2 rho) P|V|.
dv        P^T dO with P recomputed (rho) and rounded to bf16 (u), n = L.
dS        P (dP - D): (u + rho)|dS| for P and the bf16 rounding of dS as MFMA
          operand; dP and D are HD products each in fp32, then a difference
          and a product: (HD+4) 2^-23 P (|dO||V|^T + |dO|.|O|).
dq, dk    scale * dS K and scale * dS^T Q, n = L, inheriting E_dS through
          |K| and |Q|.
The kernels have no other rounding point: P and dS exist only in registers,
and the exchange that builds the 16-byte stores moves bf16 bits unchanged.
"""

import torch

import kernel_bounds as kb

BF16, F32 = torch.bfloat16, torch.float32
U = kb.U_OUT[BF16]


def _split(t, heads, n):
    """[C, B, L, n*H] -> n fp64 tensors [CB, heads, L, HD]."""
    C, B, L, W = t.shape
    return kb.upcast(t).reshape(C * B, L, n, heads, W // (n * heads)) \
        .permute(2, 0, 3, 1, 4)


def _merge(x):
    """[CB, heads, L, HD] -> [CB, L, heads*HD]."""
    return x.permute(0, 2, 1, 3).reshape(x.shape[0], x.shape[2], -1)


def _scores(q, k):
    HD, L = q.shape[-1], q.shape[-2]
    scale = HD ** -0.5
    live = torch.ones(L, L, dtype=torch.bool).tril()
    s = (scale * q @ k.transpose(-1, -2)).masked_fill(~live, float("-inf"))
    e_s = (HD + 3) * kb.U_ACC * scale * (q.abs() @ k.abs().transpose(-1, -2))
    e_max = e_s.masked_fill(~live, 0.0).amax(dim=-1, keepdim=True)
    return s, scale, e_max, 2 * e_max + kb.U_INTRINSIC


def check_forward(qkv, heads, att, lse, label):
    q, k, v = _split(qkv, heads, 3)
    L = q.shape[-2]
    s, _, e_max, rho = _scores(q, k)
    m = s.amax(dim=-1, keepdim=True)
    lse_ref = s.logsumexp(dim=-1, keepdim=True)
    kb.assert_bounded(lse.unsqueeze(-1), lse_ref,
                      m.abs() + (lse_ref - m).abs() + 1.0, L, F32,
                      intrinsic=True, label=label + ".lse",
                      extra=e_max + kb.U_INTRINSIC)
    p = (s - lse_ref).exp()
    a = p @ v.abs()
    kb.assert_bounded(att.reshape(_merge(a).shape), _merge(p @ v), _merge(a),
                      2 * L, BF16, intrinsic=True, label=label + ".att",
                      extra=_merge((U + 2 * rho) * a))


def check_backward(qkv, heads, att, lse, datt, dqkv, label):
    q, k, v = _split(qkv, heads, 3)
    (o,), (do,) = _split(att, heads, 1), _split(datt, heads, 1)
    dq_k, dk_k, dv_k = _split(dqkv, heads, 3)
    HD, L = q.shape[-1], q.shape[-2]
    s, scale, _, rho = _scores(q, k)
    p = (s - kb.upcast(lse).unsqueeze(-1)).exp()
    d = (do * o).sum(dim=-1, keepdim=True)
    d_abs = (do.abs() * o.abs()).sum(dim=-1, keepdim=True)
    dp = do @ v.transpose(-1, -2)
    ds = p * (dp - d)
    e_ds = (U + rho) * ds.abs() + (HD + 4) * kb.U_ACC * p * (
        do.abs() @ v.abs().transpose(-1, -2) + d_abs)
    pt, dst = p.transpose(-1, -2), ds.transpose(-1, -2)
    kb.assert_bounded(dv_k, pt @ do, pt @ do.abs(), L, BF16, label=label + ".dv",
                      extra=((U + rho) * p).transpose(-1, -2) @ do.abs())
    kb.assert_bounded(dq_k, scale * ds @ k, scale * ds.abs() @ k.abs(), L,
                      BF16, label=label + ".dq", extra=scale * e_ds @ k.abs())
    kb.assert_bounded(dk_k, scale * dst @ q, scale * dst.abs() @ q.abs(), L,
                      BF16, label=label + ".dk",
                      extra=scale * e_ds.transpose(-1, -2) @ q.abs())
