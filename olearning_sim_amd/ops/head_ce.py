"""The tied LM head's cross-entropy between its GEMMs (csrc/head_ce.hip).

models/bert.py ``_TiedHeadCE`` walks the vocabulary in slices.  Per slice
``[s0, s0 + s)`` a bmm writes the logits tile [C, N, s]; ``head_ce_stats``
folds that tile into the per-row online-softmax state m, l, zy (fp32 [C, N],
in place) and ``head_ce_grad`` turns the recomputed tile into dlogits and
dbias[:, s0 : s0 + s], one kernel each.

``head_ce_route`` says which path a tile takes: "fused8" / "fused2" /
"fused1" (16-byte packs, 4-byte pairs, single elements, by the divisibility
of s) for a contiguous bf16 GPU tile on a 16-byte boundary; "torch" (the
eager body in models/bert.py) for everything else, CPU and fp32 included.
OLSIM_HEAD_CE=torch, read at call time, sends every slice to the library:
the A/B switch.
"""

from __future__ import annotations

import os

import torch

from .fused import load_hip_ops

# kernel launches through this module since import (tests and tools read
# the difference)
HEAD_CE_CALLS = 0


def head_ce_route(logits: torch.Tensor, bias: torch.Tensor = None) -> str:
    """The route of one slice's logits tile [C, N, s].  With ``bias`` given,
    also "torch" for a bias the kernels do not read: anything but bf16 with
    unit column stride and a client stride of 0 or V."""
    if not logits.is_cuda or \
            os.environ.get("OLSIM_HEAD_CE", "fused") == "torch":
        return "torch"
    if bias is not None and not (
            bias.dtype == torch.bfloat16 and bias.dim() == 2
            and bias.stride(1) == 1 and bias.stride(0) in (0, bias.shape[1])):
        return "torch"
    ops = load_hip_ops(required=True)
    aligned = logits.is_contiguous() and logits.data_ptr() % 16 == 0
    return ops.head_ce_route(logits.shape[-1],
                             logits.dtype == torch.bfloat16, aligned)


def head_ce_stats(logits, bias, labels, s0, m, l, zy) -> None:
    """Merge slice [s0, s0 + s) into m, l, zy in place: m the running
    maximum of z = logits + bias, l the sum of exp(z - m), zy the label's z
    where the label is in the slice.  The state starts at -inf, 0, 0."""
    global HEAD_CE_CALLS
    HEAD_CE_CALLS += 1
    load_hip_ops(required=True).head_ce_stats(logits, bias, labels, s0, m, l,
                                              zy)


def head_ce_grad(logits, bias, labels, s0, m, l, g, dbias, out=None):
    """dlogits = bf16(g * (exp(z - m - log l) - onehot)) of the slice, and
    its column sums over N into dbias[:, s0 : s0 + s] (dbias [C, V] bf16).
    ``g`` is a one-element fp32 GPU tensor, or a number (copied to the GPU).
    ``out`` may be ``logits`` itself; None allocates."""
    global HEAD_CE_CALLS
    HEAD_CE_CALLS += 1
    if not isinstance(g, torch.Tensor):
        g = torch.tensor([g], device=logits.device, dtype=torch.float32)
    if out is None:
        out = torch.empty_like(logits)
    load_hip_ops(required=True).head_ce_grad(
        logits, bias, labels, s0, m, l, g.to(torch.float32), dbias, out)
    return out
