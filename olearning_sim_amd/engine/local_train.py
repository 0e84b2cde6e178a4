"""Client-batched local training.

One call trains a *chunk* of co-resident clients for E local steps from
the current global model and accumulates their weighted deltas — the
MI355X replacement for the reference's per-phone subprocess loop
(utils_run_task.py:481-514, one `os.system` per virtual device).

Hot path per local step:
  forward/backward through the client-batched model (grouped convs /
  batched MFMA GEMMs), then ONE fused SGD/FedProx update kernel over the
  contiguous [C*P] replica buffer (ops/csrc/fused_update.hip).
After the E steps, ONE weighted-delta reduction kernel folds
(w_c - w_global) * alpha_c into the fp32 delta accumulator
(ops/csrc/aggregate.hip); with uplink compression on, the kernel that
quantises each update as it reads it (ops/csrc/uplink_quant.hip).
"""

from __future__ import annotations

from typing import Any, Dict, Optional

import torch

from ..models.base import ClientBatchedModel, Params
from ..ops import fused
from .client_manager import FlatParams, replicate_params
from .data import SyntheticFederatedData


class LocalTrainer:
    def __init__(self, model: ClientBatchedModel, master: FlatParams,
                 data: SyntheticFederatedData, lr: float, prox_mu: float,
                 local_steps: int, batch_size: int, dtype: torch.dtype,
                 report_loss: bool = True, clip_norm: float = 0.0,
                 update_norm_stats: bool = False, uplink_bits: int = 0,
                 uplink_seed: int = 0, uplink_rank: int = 0):
        # report_loss=False avoids a device sync per chunk (bench path)
        self.report_loss = report_loss
        # clip_norm > 0: each client's update is scaled to norm <= clip_norm
        # in the aggregation; update_norm_stats: the norms are computed and
        # returned even when nothing is clipped
        self.clip_norm = clip_norm
        self.update_norm_stats = update_norm_stats
        # uplink_bits > 0: the updates are quantised to that many bits per
        # weight as they are accumulated; (uplink_seed, uplink_rank) and
        # the round key the draws (fused.uplink_key)
        self.uplink_bits = uplink_bits
        self.uplink_seed = uplink_seed
        self.uplink_rank = uplink_rank
        # where each parameter starts in the flat master
        self._elem_offsets: Dict[str, int] = {}
        off = 0
        for k, n in master.numels.items():
            self._elem_offsets[k] = off
            off += n
        self.model = model
        self.master = master
        self.data = data
        self.lr = lr
        self.prox_mu = prox_mu
        self.local_steps = local_steps
        self.batch_size = batch_size
        self.dtype = dtype
        # cast of the fp32 master into the compute dtype; row-major
        # param-major layout identical to master.flat
        self._cast_flat: Optional[torch.Tensor] = None

    def begin_round(self) -> None:
        """Re-cast the master once per round (clients replicate from it)."""
        self._cast_flat = self.master.flat.to(self.dtype)

    def _cast_params(self) -> Params:
        assert self._cast_flat is not None, "begin_round() not called"
        return self.master.views_of(self._cast_flat)

    def _attach_master_wt(self, cast: Params, params: Params, C: int) -> None:
        """Give every 3x3 weight whose stride-1 dgrad runs as a forward
        convolution (ops/conv.py _dgrad_p) its flipped-transposed copy for
        the first local step.  All replicas equal the master there, so the
        copy is the repacked master replicated: a write with no read.  The
        SGD update keeps it current through the later steps
        (fused_sgd_update keep_wt) and drops it at the last."""
        import os
        wanted = getattr(self.model, "dgrad_wt_params", None)
        # OLSIM_DGRAD_WT=repack: the backward repacks w on every call and
        # no copy is held ("0" is dgrad_wt_ok's to refuse)
        if (wanted is None or self.dtype != torch.bfloat16
                or not self._cast_flat.is_cuda
                or os.environ.get("OLSIM_DGRAD_WT", "1") == "repack"):
            return
        from ..ops.conv import attach_wt, dgrad_wt_ok
        ops = fused.load_hip_ops(required=True)
        for k, (H, W) in wanted(cast).items():
            OC, IC = cast[k].shape[0], cast[k].shape[1]
            # no copy where the backward would not read it
            if not dgrad_wt_ok(ops, OC, IC, self.batch_size, H, W):
                continue
            # clone: cast[k] is a view into the flat cast at any 2-byte
            # offset, the kernel loads 16 bytes at a time
            wt0 = ops.conv3x3_wflip(cast[k].detach().clone()[None])[0]
            attach_wt(params[k], ops.replicate(wt0, C))

    def train_chunk(self, client_ids: torch.Tensor, weights: torch.Tensor,
                    round_idx: int, delta_flat: torch.Tensor,
                    wsum: Optional[float] = None) -> Dict[str, Any]:
        """Train one chunk of clients; accumulate weighted deltas.

        client_ids: [C] int64; weights: [C] fp32 aggregation weights
        (0 for clients whose gradient the behaviour model drops);
        delta_flat: fp32 [P] accumulator with the master's layout.

        With clipping or norm statistics on, the result also carries "sq"
        (fp32 [C], each client's squared update norm) and "weights", both
        on the device and not read here.
        """
        C = int(client_ids.numel())
        cast = self._cast_params()
        params = replicate_params(cast, C)
        plist = list(params.values())
        glist = [cast[k] for k in params]
        self._attach_master_wt(cast, params, C)
        last_loss = 0.0
        for step in range(self.local_steps):
            x, y = self.data.batch(client_ids, round_idx, step,
                                   self.batch_size, self.dtype)
            loss = self.model.loss(params, x, y)
            # loss is the mean over C*B rows; each client's SGD step needs
            # the gradient of ITS OWN per-client mean, i.e. d(loss*C)/dw_c
            # — this also makes training invariant to the chunking.
            grads = torch.autograd.grad(loss * C, plist, allow_unused=True)
            with torch.no_grad():
                live = [(p, g) for p, g in zip(plist, grads) if g is not None]
                fused.fused_sgd_update(
                    [p for p, _ in live], [g for _, g in live],
                    lr=self.lr, mu=self.prox_mu,
                    global_params=[cast[k] for k, g in
                                   zip(params, grads) if g is not None],
                    keep_wt=step < self.local_steps - 1)
            if self.report_loss and step == self.local_steps - 1:
                last_loss = float(loss.detach())
            del grads
        out: Dict[str, Any] = {"loss": last_loss, "clients": C}
        with torch.no_grad():
            delta_views = list(self.master.views_of(delta_flat).values())
            final = [p.detach() for p in plist]
            if self.clip_norm > 0.0 or self.update_norm_stats:
                sq = fused.client_delta_sqnorm(final, glist)
                out["sq"], out["weights"] = sq, weights
                if self.clip_norm > 0.0:
                    # s_c = min(1, S/||delta_c||) folds into the weights;
                    # their sum stays on the device for the accumulate
                    weights, wsum = fused.clip_weights(sq, weights,
                                                       self.clip_norm)
            if self.uplink_bits > 0:
                # nothing is hoisted: no wsum.  The clip factor in the
                # weights scales the quantised update (the quantiser is
                # scale-equivariant).
                fused.weighted_delta_accum_quant(
                    delta_views, final, glist, weights, client_ids,
                    self.uplink_bits,
                    fused.uplink_key(self.uplink_seed, round_idx,
                                     self.uplink_rank),
                    [self._elem_offsets[k] for k in params])
            else:
                fused.weighted_delta_accum(
                    delta_views, final, glist, weights,
                    wsum=wsum if wsum is not None else float(weights.sum()))
        return out
