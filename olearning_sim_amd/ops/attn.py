"""Fused causal self-attention of the per-client BERT (csrc/attn.hip).

``causal_attention(qkv, heads) -> att`` takes the packed output of the qkv
blinear viewed as [C, B, L, 3H] (q | k | v along 3H, each heads x HD) and
returns att [C, B, L, H] in the layout the attn_out blinear reads: no
permute, no transpose copy, and the backward writes dqkv packed.  One
workgroup owns one (client x batch row, head).

``attn_route`` says which path a layer takes: "fused" for bf16 GPU
operands with 1 <= L <= 128 and HD 32 or 64, contiguous and 16-byte
aligned; "torch" (scaled_dot_product_attention in models/bert.py) for
everything else, CPU tensors included.  OLSIM_ATTN=torch, read at call
time, sends every layer to the library: the A/B switch.

Sequences of 129 to 512 tokens have kernels of their own (csrc/
attn_long.hip): ``attn_long_route`` says "long" for them under the same
conditions, and ``causal_attention_long`` is the same function on those
kernels.  A model asks ``attn_route`` first and ``attn_long_route`` second.
OLSIM_ATTN_LONG=torch sends only these lengths to the library.
"""

from __future__ import annotations

import os

import torch

from .fused import load_hip_ops

# calls of causal_attention since import (tests and tools read the difference)
ATTN_CALLS = 0
# ... and of causal_attention_long
ATTN_LONG_CALLS = 0


def attn_route(qkv: torch.Tensor, heads: int) -> str:
    """"fused" or "torch" for one layer's qkv [..., L, 3*heads*HD]."""
    if not qkv.is_cuda or os.environ.get("OLSIM_ATTN", "fused") == "torch":
        return "torch"
    ops = load_hip_ops(required=True)
    aligned = qkv.is_contiguous() and qkv.data_ptr() % 16 == 0
    return ops.attn_route(qkv.shape[-2], qkv.shape[-1] // (3 * heads),
                          qkv.dtype == torch.bfloat16, aligned)


def attn_forward(qkv, heads, att=None, lse=None):
    """The forward kernel on its own: returns (att, lse), written into the
    given tensors where a caller provides them."""
    C, B, L, H3 = qkv.shape
    if att is None:
        att = torch.empty(C, B, L, H3 // 3, device=qkv.device, dtype=qkv.dtype)
    if lse is None:
        lse = torch.empty(C * B, heads, L, device=qkv.device,
                          dtype=torch.float32)
    load_hip_ops(required=True).attn_fwd(qkv, att, lse, heads)
    return att, lse


def attn_backward(datt, qkv, att, lse, heads, dqkv=None):
    """dqkv, packed like qkv, for upstream datt.  The kernel writes every
    element of it."""
    if dqkv is None:
        dqkv = torch.empty_like(qkv)
    load_hip_ops(required=True).attn_bwd(qkv, att, datt, lse, dqkv, heads)
    return dqkv


class _CausalAttentionFn(torch.autograd.Function):

    @staticmethod
    def forward(ctx, qkv, heads):
        att, lse = attn_forward(qkv, heads)
        ctx.save_for_backward(qkv, att, lse)
        ctx.heads = heads
        return att

    @staticmethod
    def backward(ctx, datt):
        qkv, att, lse = ctx.saved_tensors
        return attn_backward(datt.contiguous(), qkv, att, lse, ctx.heads), None


def causal_attention(qkv: torch.Tensor, heads: int) -> torch.Tensor:
    """att [C, B, L, H] of qkv [C, B, L, 3H] on the fused kernels.  The
    operand must be one attn_route calls "fused"; anything else raises in
    the binding."""
    global ATTN_CALLS
    ATTN_CALLS += 1
    return _CausalAttentionFn.apply(qkv, heads)


def attn_long_route(qkv: torch.Tensor, heads: int) -> str:
    """"long" or "torch" for one layer's qkv [..., L, 3*heads*HD]."""
    if (not qkv.is_cuda or os.environ.get("OLSIM_ATTN", "fused") == "torch"
            or os.environ.get("OLSIM_ATTN_LONG", "fused") == "torch"):
        return "torch"
    ops = load_hip_ops(required=True)
    aligned = qkv.is_contiguous() and qkv.data_ptr() % 16 == 0
    return ops.attn_long_route(qkv.shape[-2], qkv.shape[-1] // (3 * heads),
                               qkv.dtype == torch.bfloat16, aligned)


def attn_long_forward(qkv, heads, att=None, lse=None):
    """attn_forward on the kernels for 129 <= L <= 512."""
    C, B, L, H3 = qkv.shape
    if att is None:
        att = torch.empty(C, B, L, H3 // 3, device=qkv.device, dtype=qkv.dtype)
    if lse is None:
        lse = torch.empty(C * B, heads, L, device=qkv.device,
                          dtype=torch.float32)
    load_hip_ops(required=True).attn_long_fwd(qkv, att, lse, heads)
    return att, lse


def attn_long_backward(datt, qkv, att, lse, heads, dqkv=None, dsum=None):
    """attn_backward on the kernels for 129 <= L <= 512: a row-dot kernel
    fills dsum (dO_i . O_i, shaped like lse), then one kernel writes every
    element of dqkv."""
    if dqkv is None:
        dqkv = torch.empty_like(qkv)
    if dsum is None:
        dsum = torch.empty_like(lse)
    load_hip_ops(required=True).attn_long_bwd(qkv, att, datt, lse, dsum, dqkv,
                                              heads)
    return dqkv


class _CausalAttentionLongFn(torch.autograd.Function):

    @staticmethod
    def forward(ctx, qkv, heads):
        att, lse = attn_long_forward(qkv, heads)
        ctx.save_for_backward(qkv, att, lse)
        ctx.heads = heads
        return att

    @staticmethod
    def backward(ctx, datt):
        qkv, att, lse = ctx.saved_tensors
        return attn_long_backward(datt.contiguous(), qkv, att, lse,
                                  ctx.heads), None


def causal_attention_long(qkv: torch.Tensor, heads: int) -> torch.Tensor:
    """causal_attention for an operand attn_long_route calls "long";
    anything else raises in the binding."""
    global ATTN_LONG_CALLS
    ATTN_LONG_CALLS += 1
    return _CausalAttentionLongFn.apply(qkv, heads)
