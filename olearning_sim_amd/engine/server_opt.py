"""Server optimiser state: FedAvgM and the FedOpt family on the flat master.

The round's reduced delta is a pseudo-gradient (Reddi et al., "Adaptive
Federated Optimization", Algorithm 2; Hsu et al. for server momentum):

    g = delta / total_weight + sigma * noise

and the master takes an optimiser step on it instead of the plain
``master += delta / total_weight``.  The rule itself is
``ops.fused.server_opt_step``; this class owns what the rule carries from
round to round: m (all kinds), v (adagrad, adam, yogi) and the number of
steps taken.  State is fp32 in the layout of ``master.flat``.  Every rank
sees the same delta, weight and noise, so every rank takes the same step
and the state is never communicated.
"""

from __future__ import annotations

from typing import Dict, Optional

import torch

from ..ops import fused

KINDS = fused.SERVER_OPT_KINDS
ADAPTIVE = ("adagrad", "adam", "yogi")


def validate(kind: str, lr: float, beta1: float, beta2: float,
             tau: float) -> None:
    """ValueError on a setting no rule is defined for ("" = off is the
    caller's to handle)."""
    if kind not in KINDS:
        raise ValueError(f"server_optimizer {kind!r} not one of "
                         f"{('',) + KINDS}")
    if not lr > 0:
        raise ValueError("server_lr must be > 0")
    for name, b in (("server_beta1", beta1), ("server_beta2", beta2)):
        if not 0 <= b < 1:
            raise ValueError(f"{name} must be in [0, 1)")
    if kind in ADAPTIVE and not tau > 0:
        raise ValueError("server_tau must be > 0")


class ServerOptimizer:
    def __init__(self, kind: str, numel: int, device, lr: float = 1.0,
                 beta1: float = 0.9, beta2: float = 0.99,
                 tau: float = 1e-3):
        validate(kind, lr, beta1, beta2, tau)
        self.kind = kind
        self.lr, self.beta1, self.beta2, self.tau = lr, beta1, beta2, tau
        # m0 = 0; v0 = tau^2 in every element (FedOpt's initial
        # accumulator, so the first denominator is 2*tau at g = 0)
        self.m = torch.zeros(numel, dtype=torch.float32, device=device)
        self.v: Optional[torch.Tensor] = None
        if kind in ADAPTIVE:
            self.v = torch.full((numel,), tau * tau, dtype=torch.float32,
                                device=device)
        self.steps = 0

    def step(self, master_flat: torch.Tensor, delta: torch.Tensor,
             total_weight: float, noise: Optional[torch.Tensor] = None,
             sigma: float = 0.0) -> None:
        """One step on master_flat, in place.  A round without weight
        takes none: master, m, v and the count stay as they were."""
        if not total_weight > 0:
            return
        fused.server_opt_step(self.kind, master_flat, delta, self.m, self.v,
                              total_weight, self.lr, self.beta1, self.beta2,
                              self.tau, noise=noise, sigma=sigma)
        self.steps += 1

    def state_dict(self) -> Dict[str, torch.Tensor]:
        sd = {"m": self.m, "step": torch.tensor([self.steps],
                                                dtype=torch.int64)}
        if self.v is not None:
            sd["v"] = self.v
        return sd

    def load_state_dict(self, sd: Dict[str, torch.Tensor]) -> None:
        want = {"m", "step"} | ({"v"} if self.v is not None else set())
        if set(sd) != want:
            raise ValueError(f"server optimiser state has {sorted(sd)}, "
                             f"{self.kind!r} needs {sorted(want)}")
        for name in want - {"step"}:
            mine = getattr(self, name)
            if sd[name].shape != mine.shape:
                raise ValueError(f"server optimiser state {name!r} has "
                                 f"shape {tuple(sd[name].shape)}, expected "
                                 f"{tuple(mine.shape)}")
            mine.copy_(sd[name])
        self.steps = int(sd["step"].reshape(-1)[0])
