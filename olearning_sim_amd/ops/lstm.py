"""Fused per-client LSTM recurrence (csrc/lstm.hip).

``lstm_layer(xp, w_hh) -> hs`` runs one layer's recurrence over the whole
sequence from zero initial state: xp [C, B, L, 4H] is the hoisted input
projection (bias included, gate order i | f | g | o), w_hh [C, H, 4H].
One workgroup owns one client for all L steps; h and c stay on chip.

``lstm_route`` says which path a layer takes: "fused" for bf16 GPU
operands with 1 <= B <= 16, H a multiple of 64 up to 256, contiguous and
16-byte aligned; "torch" (the per-timestep loop in models/lstm.py) for
everything else, CPU tensors included.  OLSIM_LSTM=torch, read at call
time, sends every layer to the torch loop: the A/B switch.
"""

from __future__ import annotations

import os

import torch

from .fused import fast_transpose, load_hip_ops

# calls of lstm_layer since import (tests and tools read the difference)
LAYER_CALLS = 0


def lstm_route(xp: torch.Tensor, w_hh: torch.Tensor) -> str:
    """"fused" or "torch" for one layer's operands."""
    if not xp.is_cuda or os.environ.get("OLSIM_LSTM", "fused") == "torch":
        return "torch"
    ops = load_hip_ops(required=True)
    is_bf16 = xp.dtype == torch.bfloat16 and w_hh.dtype == torch.bfloat16
    aligned = all(t.is_contiguous() and t.data_ptr() % 16 == 0
                  for t in (xp, w_hh))
    return ops.lstm_route(xp.shape[1], w_hh.shape[1], is_bf16, aligned)


def lstm_forward(xp, w_hh, hs=None, gates=None, cs=None):
    """The forward kernel on its own: returns (hs, gates, cs), written into
    the given tensors where a caller provides them."""
    C, B, L, H4 = xp.shape
    H = H4 // 4
    if hs is None:
        hs = torch.empty(C, B, L, H, device=xp.device, dtype=xp.dtype)
    if gates is None:
        gates = torch.empty_like(xp)
    if cs is None:
        cs = torch.empty(C, B, L, H, device=xp.device, dtype=torch.float32)
    load_hip_ops(required=True).lstm_fwd(xp, w_hh, hs, gates, cs)
    return hs, gates, cs


def lstm_backward(dhs, gates, cs, hs, w_hh, dgates=None):
    """(dgates, dW_hh) for upstream dhs.  dgates [C, B, L, 4H] comes from
    the backward kernel and is the gradient of xp; dW_hh = h_prev^T dgates
    is one bmm over B*L whose operands are both materialised (hipBLASLt
    faults on strided and transposed views, see models/base.py)."""
    C, B, L, H = hs.shape
    if dgates is None:
        dgates = torch.empty_like(gates)
    load_hip_ops(required=True).lstm_bwd(dhs, gates, cs, w_hh, dgates)
    h_prev = torch.zeros_like(hs)
    h_prev[:, :, 1:] = hs[:, :, :-1]
    dw = torch.bmm(fast_transpose(h_prev.view(C, B * L, H)),
                   dgates.view(C, B * L, 4 * H))
    return dgates, dw


class _LstmLayerFn(torch.autograd.Function):

    @staticmethod
    def forward(ctx, xp, w_hh):
        hs, gates, cs = lstm_forward(xp, w_hh)
        ctx.save_for_backward(gates, cs, hs, w_hh)
        return hs

    @staticmethod
    def backward(ctx, dhs):
        gates, cs, hs, w_hh = ctx.saved_tensors
        return lstm_backward(dhs.contiguous(), gates, cs, hs, w_hh)


def lstm_layer(xp: torch.Tensor, w_hh: torch.Tensor) -> torch.Tensor:
    """hs [C, B, L, H] of one LSTM layer on the fused kernels.  The
    operands must be ones lstm_route calls "fused"; anything else raises
    in the binding."""
    global LAYER_CALLS
    LAYER_CALLS += 1
    return _LstmLayerFn.apply(xp, w_hh)
