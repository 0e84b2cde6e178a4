"""Bounds of the long-sequence attention kernels (ops/csrc/attn_long.hip),
on top of attn_ref.py, whose rounding points all carry over: the scores, the
probabilities and the products are formed the same way, and the backward
takes P from lse exactly as the short kernel does, so
``attn_ref.check_backward`` holds unchanged (D now comes from a kernel of
its own: HD products in fp32, the term attn_ref already carries; dQ, dK and
dV accumulate over key or query blocks in fp32 registers, n = L as before).

The forward's online softmax adds, for nb = ceil(L / 128) key blocks:

lse  l <- l * alpha + rowsum at each of up to nb - 1 later blocks.  alpha =
     exp2((m - m_new) log2e) is one fast exp2 (2^-16 relative, its argument
     scaling included) and the product and the sum round once each in fp32
     (2 * 2^-24 = 2^-23).  Relative on l, hence absolute on lse = m +
     log(l):  extra = (nb - 1) (2^-16 + 2^-23).
att  the O^T accumulators of a query and its l are multiplied by the same
     value alpha in the same lane, so alpha's own error cancels in O / l;
     what remains is one fp32 rounding per multiplication on each side:
     n = 2 L + 2 (nb - 1).
"""

import attn_ref
import kernel_bounds as kb

BLOCK = 128


def check_forward(qkv, heads, att, lse, label):
    q, k, v = attn_ref._split(qkv, heads, 3)
    L = q.shape[-2]
    nb = -(-L // BLOCK)
    s, _, e_max, rho = attn_ref._scores(q, k)
    m = s.amax(dim=-1, keepdim=True)
    lse_ref = s.logsumexp(dim=-1, keepdim=True)
    kb.assert_bounded(lse.unsqueeze(-1), lse_ref,
                      m.abs() + (lse_ref - m).abs() + 1.0, L, attn_ref.F32,
                      intrinsic=True, label=label + ".lse",
                      extra=e_max + kb.U_INTRINSIC
                      + (nb - 1) * (kb.U_INTRINSIC + kb.U_ACC))
    p = (s - lse_ref).exp()
    a = p @ v.abs()
    merge = attn_ref._merge
    kb.assert_bounded(att.reshape(merge(a).shape), merge(p @ v), merge(a),
                      2 * L + 2 * (nb - 1), attn_ref.BF16, intrinsic=True,
                      label=label + ".att",
                      extra=merge((attn_ref.U + 2 * rho) * a))


check_backward = attn_ref.check_backward
