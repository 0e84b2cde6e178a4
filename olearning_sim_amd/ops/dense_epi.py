"""What follows the bias-free GEMMs of a BertLM encoder layer
(csrc/dense_epi.hip).

``bias_gelu(z, b)`` is gelu(z + b) (erf form) for ffn_in, and
``bias_residual_layernorm(z, b, res, gamma, beta)`` is LayerNorm(z + b + res)
* gamma + beta for attn_out and ffn_out: one kernel forward, and backward one
kernel plus the shared column-sum finish, where the library runs a bias pass,
a residual pass, the activation or the LayerNorm, and a reduction per bias.
The backward's bias, gamma and beta gradients are summed in a fixed order
(no atomics): two runs give the same bits.

``dense_epi_route`` says which path a call takes: "fused" for contiguous bf16
GPU operands on 16-byte boundaries whose last dimension is a multiple of 8
(and, with a residual, at most 1536); "torch" (the lines in models/bert.py)
for everything else, CPU and fp32 included.  OLSIM_DENSE_EPI=fused|torch,
read at call time, is the A/B switch; unset, DEFAULT_ROUTE decides
(profiles/dense_epi_r16.md).
"""

from __future__ import annotations

import os

import torch

from .fused import load_hip_ops

# kernel launches through this module since import (tests and tools read the
# difference): 1 per forward op, 2 per backward op (kernel + column finish)
DENSE_EPI_CALLS = 0

DEFAULT_ROUTE = "fused"

# rows per workgroup of the kernels that build column sums
# (profiles/dense_epi_r16.md has the comparison)
GELU_ROWS = 32
LN_ROWS = 32

BF16 = torch.bfloat16


def _operand_ok(t, shape) -> bool:
    return t.is_cuda and t.dtype == BF16 and t.shape == shape \
        and t.is_contiguous() and t.data_ptr() % 16 == 0


def dense_epi_route(z: torch.Tensor, b: torch.Tensor,
                    res: torch.Tensor = None, gamma: torch.Tensor = None,
                    beta: torch.Tensor = None) -> str:
    """The route of one epilogue on z [C, N, W] with bias b [C, W]: the GELU
    form, or with ``res`` (and gamma, beta) the LayerNorm form."""
    if not z.is_cuda or z.dim() != 3 or \
            os.environ.get("OLSIM_DENSE_EPI", DEFAULT_ROUTE) == "torch":
        return "torch"
    C, _, W = z.shape
    aligned = z.is_contiguous() and z.data_ptr() % 16 == 0
    for col in (b, gamma, beta):
        if col is not None and not _operand_ok(col, (C, W)):
            return "torch"
    if res is not None and not _operand_ok(res, z.shape):
        return "torch"
    return load_hip_ops(required=True).dense_epi_route(
        W, z.dtype == BF16, aligned, res is not None)


def _grad_operand(dy):
    dy = dy.contiguous()
    return dy if dy.data_ptr() % 16 == 0 else dy.clone()


def bias_gelu_fwd(z, b, out=None):
    """out <- bf16(gelu(f32(z) + f32(b))); None allocates."""
    global DENSE_EPI_CALLS
    DENSE_EPI_CALLS += 1
    out = torch.empty_like(z) if out is None else out
    load_hip_ops(required=True).bias_gelu_fwd(z, b, out, GELU_ROWS)
    return out


def bias_gelu_bwd(z, b, dy, dz=None, db=None):
    """dz <- bf16(dy * gelu'(z + b)) and db [1, C, F] <- the fp32 column sums
    of the rounded dz, stored as bf16.  Returns (dz, db)."""
    global DENSE_EPI_CALLS
    DENSE_EPI_CALLS += 2
    dz = torch.empty_like(z) if dz is None else dz
    db = b.new_empty((1,) + b.shape) if db is None else db
    load_hip_ops(required=True).bias_gelu_bwd(z, b, dy, dz, db, GELU_ROWS)
    return dz, db


def brln_fwd(z, b, res, gamma, beta, eps, y=None, s=None, mean=None,
             rstd=None):
    """s <- bf16(z + b + res); mean, rstd of the rounded s over the last
    dimension; y <- bf16((s - mean) * rstd * gamma + beta)."""
    global DENSE_EPI_CALLS
    DENSE_EPI_CALLS += 1
    y = torch.empty_like(z) if y is None else y
    s = torch.empty_like(z) if s is None else s
    stat = dict(device=z.device, dtype=torch.float32)
    mean = torch.empty(z.shape[:2], **stat) if mean is None else mean
    rstd = torch.empty(z.shape[:2], **stat) if rstd is None else rstd
    load_hip_ops(required=True).brln_fwd(z, b, res, gamma, beta, eps, y, s,
                                         mean, rstd)
    return y, s, mean, rstd


def brln_bwd(s, dy, gamma, mean, rstd, ds=None, cols=None):
    """ds <- the gradient of s (of z and of res alike) and cols [3, C, H] <-
    dgamma, dbeta, db as bf16.  Returns (ds, cols)."""
    global DENSE_EPI_CALLS
    DENSE_EPI_CALLS += 2
    ds = torch.empty_like(s) if ds is None else ds
    cols = gamma.new_empty((3,) + gamma.shape) if cols is None else cols
    load_hip_ops(required=True).brln_bwd(s, dy, gamma, mean, rstd, ds, cols,
                                         LN_ROWS)
    return ds, cols


class _BiasGelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, b):
        ctx.save_for_backward(z, b)
        return bias_gelu_fwd(z, b)

    @staticmethod
    def backward(ctx, dy):
        z, b = ctx.saved_tensors
        dz, db = bias_gelu_bwd(z, b, _grad_operand(dy))
        return dz, db[0]


class _BiasResidualLayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, b, res, gamma, beta, eps):
        y, s, mean, rstd = brln_fwd(z, b, res, gamma, beta, eps)
        ctx.save_for_backward(s, gamma, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        s, gamma, mean, rstd = ctx.saved_tensors
        ds, cols = brln_bwd(s, _grad_operand(dy), gamma, mean, rstd)
        # z and res enter s with weight one: one tensor is both gradients
        return ds, cols[2], ds, cols[0], cols[1], None


def bias_gelu(z: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """gelu(z + b), z [C, N, F] the bias-free output of blinear, b [C, F].
    For operands on the "fused" route; anything else is an error."""
    return _BiasGelu.apply(z, b)


def bias_residual_layernorm(z: torch.Tensor, b: torch.Tensor,
                            res: torch.Tensor, gamma: torch.Tensor,
                            beta: torch.Tensor,
                            eps: float = 1e-5) -> torch.Tensor:
    """LayerNorm(z + b + res) * gamma + beta over the last dimension; z, res
    [C, N, H], b, gamma, beta [C, H].  For operands on the "fused" route."""
    return _BiasResidualLayerNorm.apply(z, b, res, gamma, beta, eps)
