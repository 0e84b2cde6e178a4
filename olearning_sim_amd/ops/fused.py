"""Python surface of the fused HIP ops.

Replaces the per-device subprocess training loop of the reference
(ols_core/taskMgr/utils/utils_run_task.py:481-514) with client-batched
device kernels.  Three bandwidth-bound fused ops carry the optimizer/
aggregation tail of every local-train step:

- fused_sgd_update:      w_c -= lr * (g_c + mu * (w_c - w_global))
                         (mu=0 -> FedAvg local SGD; mu>0 -> FedProx)
- weighted_delta_accum:  delta += sum_c alpha_c * (w_c - w_global)
- weighted_delta_accum_quant: the same sum over updates quantised to 2, 4
                         or 8 bits per weight as they are read (uplink
                         compression)
- apply_aggregate:       w_global += delta / total_weight  (fp32 master)
- server_opt_step:       FedAvgM / FedAdagrad / FedAdam / FedYogi step on
                         the fp32 master with g = delta / total_weight
                         [+ sigma * noise], m and v in place, one launch
- cross_entropy_fwd_bwd: fused softmax CE loss + dlogits in one pass

On ROCm these run as hand-written gfx950 kernels (csrc/*.hip, bf16x8 per
lane); on CPU they fall back to eager torch so the control-plane tests
run here.  A CUDA tensor with no extension raises (no silent fallback).
"""

from __future__ import annotations

import os
from typing import Optional, Sequence, Union

import torch

_HIP_OPS = None
_HIP_OPS_TRIED = False

_SO_NAME = "_hip_ops.so"


def _so_path() -> str:
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), _SO_NAME)


def load_hip_ops(required: bool = False):
    """Load the in-tree extension if built. Caches the result."""
    global _HIP_OPS, _HIP_OPS_TRIED
    if _HIP_OPS is not None:
        return _HIP_OPS
    if _HIP_OPS_TRIED and not required:
        return None
    _HIP_OPS_TRIED = True
    path = _so_path()
    if os.path.exists(path):
        torch.ops.load_library(path)
        _HIP_OPS = torch.ops.olsim_hip
        return _HIP_OPS
    if required:
        raise RuntimeError(
            f"olearning_sim_amd HIP extension missing: {path} not built. "
            f"Run `python -m olearning_sim_amd.ops.build` (hipcc, gfx950).")
    return None


def hip_ops_available() -> bool:
    return load_hip_ops() is not None


_OFFS_CACHE = {}
_EMPTY_OFFS = None


def _cached_offsets(n: int, device) -> torch.Tensor:
    """[0, n] block table, cached — avoids a tiny H2D copy per
    parameter per step in the list-form fused ops."""
    key = (n, str(device))
    t = _OFFS_CACHE.get(key)
    if t is None:
        t = torch.tensor([0, n], dtype=torch.int64, device=device)
        _OFFS_CACHE[key] = t
    return t


def _gpu_ops(t: torch.Tensor):
    """Return the HIP op namespace for a GPU tensor; raise if unavailable."""
    if t.is_cuda:
        return load_hip_ops(required=True)
    return None


def _wt_update_ok(w: torch.Tensor, g: torch.Tensor) -> bool:
    """What sgd_conv3_wt asks of w and g beyond their shape (a wt was
    attached, so the shape passed conv3x3_wflip): anything else takes the
    plain update and loses the copy."""
    return all(t.dtype == torch.bfloat16 and t.is_contiguous()
               and t.data_ptr() % 16 == 0 for t in (w, g))


# ---------------------------------------------------------------------------
def fused_sgd_update(params: Sequence[torch.Tensor],
                     grads: Sequence[torch.Tensor],
                     lr: float,
                     mu: float = 0.0,
                     global_params: Optional[Sequence[torch.Tensor]] = None,
                     keep_wt: bool = False) -> None:
    """In-place SGD / FedProx step over per-client parameter tensors.

    params[i]: [C, ...] client replicas; grads[i] same shape;
    global_params[i]: [...] (no client dim) — required when mu > 0.

    A 3x3 conv weight may carry a flipped-transposed copy for its dgrad
    (ops/conv.py attach_wt).  With keep_wt and mu == 0 such a weight takes
    the update kernel that rewrites the copy from the values it has just
    computed (conv3_wflip.hip k_sgd_conv3_wt), so the copy stays current;
    otherwise the copy is dropped before w changes.
    """
    if not params:
        return
    if params[0].is_cuda:
        from .conv import _live_wt, attach_wt, drop_wt
        for i, (w, g) in enumerate(zip(params, grads)):
            held = getattr(w, "_olsim_wt", None)
            if held is not None:
                wt = _live_wt(held, w) if keep_wt and mu == 0.0 else None
                drop_wt(w)
                if wt is not None and _wt_update_ok(w, g):
                    load_hip_ops(required=True).sgd_conv3_wt(w, g, wt, lr)
                    attach_wt(w, wt)
                    continue
            n = w[0].numel() if w.dim() > 1 else w.numel()
            gl = (global_params[i].reshape(-1) if (global_params is not None
                                                  and mu != 0.0)
                  else torch.empty(0, dtype=w.dtype, device=w.device))
            offs = (_cached_offsets(n, w.device) if mu != 0.0
                    else _cached_offsets(0, w.device)[:0])
            fused_sgd_update_flat(w.reshape(-1), g.reshape(-1), gl,
                                  w.shape[0], lr, mu, offs)
        return
    with torch.no_grad():
        for i, (w, g) in enumerate(zip(params, grads)):
            upd = g
            if mu != 0.0 and global_params is not None:
                upd = g + mu * (w - global_params[i].to(w.dtype))
            w.add_(upd, alpha=-lr)


def weighted_delta_accum(delta: Sequence[torch.Tensor],
                         client_params: Sequence[torch.Tensor],
                         global_params: Sequence[torch.Tensor],
                         weights: torch.Tensor,
                         wsum: Union[float, torch.Tensor, None] = None
                         ) -> None:
    """delta[i] (fp32, shape [...]) += sum_c weights[c] * (client_params[i][c] - global[i]).

    wsum: sum of the weights as a host float, or as a one-element fp32
    device tensor (clip_weights' wsum_eff), which the kernels read on the
    device."""
    if not delta:
        return
    if client_params[0].is_cuda:
        if wsum is None:
            wsum = float(weights.sum())
        for dl, cw, gw in zip(delta, client_params, global_params):
            offs = _cached_offsets(gw.numel(), cw.device)
            weighted_delta_accum_flat(dl.reshape(-1), cw.reshape(-1),
                                      gw.reshape(-1), weights, cw.shape[0],
                                      offs, wsum)
        return
    with torch.no_grad():
        for dl, cw, gw in zip(delta, client_params, global_params):
            diff = cw.float() - gw.float().unsqueeze(0)
            shape = [-1] + [1] * (cw.dim() - 1)
            dl.add_((diff * weights.view(shape)).sum(dim=0))


def client_delta_sqnorm(client_params: Sequence[torch.Tensor],
                        global_params: Sequence[torch.Tensor]) -> torch.Tensor:
    """sq[c] = sum_i ||client_params[i][c] - global_params[i]||^2 as fp32
    [C]: each client's squared update norm over all parameters.  The
    difference is taken per element in fp32.  GPU: one deterministic
    reduction per parameter (csrc/clip.hip), no host read."""
    C = client_params[0].shape[0]
    dev = client_params[0].device
    sq = torch.zeros(C, dtype=torch.float32, device=dev)
    if client_params[0].is_cuda:
        ops = load_hip_ops(required=True)
        for cw, gw in zip(client_params, global_params):
            ops.client_delta_sqnorm(sq, cw.detach().reshape(-1),
                                    gw.detach().reshape(-1), C)
        return sq
    with torch.no_grad():
        for cw, gw in zip(client_params, global_params):
            diff = cw.float() - gw.float().unsqueeze(0)
            sq.add_((diff * diff).reshape(C, -1).sum(dim=1))
    return sq


def clip_weights(sq: torch.Tensor, weights: torch.Tensor, clip_norm: float):
    """Aggregation weights of norm-clipped updates.  With s_c = S /
    sqrt(sq[c]) where sq[c] > S^2 and 1 elsewhere (S = clip_norm in fp32),
    returns (w_eff, wsum_eff): w_eff[c] = weights[c] * s_c as fp32 [C] and
    their sum as fp32 [1], both on sq's device."""
    if sq.is_cuda:
        ops = load_hip_ops(required=True)
        return ops.clip_weights(sq, weights.float().contiguous(),
                                float(clip_norm))
    with torch.no_grad():
        S = torch.tensor(float(clip_norm), dtype=torch.float32)
        s = torch.where(sq > S * S, S / sq.sqrt(), torch.ones_like(sq))
        w_eff = weights.float() * s
        return w_eff, w_eff.sum().reshape(1)


# -- uplink compression -----------------------------------------------------
#
# Each client's update is quantised to `bits` bits per weight before it is
# aggregated: per parameter tensor and per bucket of UPLINK_BUCKET
# consecutive elements, with L = 2^(bits-1) - 1 levels per sign,
#
#   d = f32(client) - f32(global)            a = max |d| over the bucket
#   t = |d| * L / a                          l = min(L, floor(t) + [u < frac(t)])
#   Q = sign(d) * l * (a / L)                (a == 0: Q = 0)
#
# u is 16 bits of a counter hash of (key, client id, element index in the
# flat master): uplink_uniform.  The quantiser is unbiased, E[Q] = d.

UPLINK_BUCKET = 512
UPLINK_BITS = (2, 4, 8)
_M32 = 0xFFFFFFFF


def uplink_levels(bits: int) -> int:
    if bits not in UPLINK_BITS:
        raise ValueError(f"uplink bits {bits!r} not one of {UPLINK_BITS}")
    return (1 << (bits - 1)) - 1


def _mul32(x: torch.Tensor, k: int) -> torch.Tensor:
    """x * k mod 2^32 on an int64 tensor of 32-bit words, formed from
    16-bit halves: a 32 x 32 bit product does not fit int64."""
    lo = (x & 0xFFFF) * k
    hi = ((x >> 16) * (k & 0xFFFF)) & 0xFFFF
    return (lo + (hi << 16)) & _M32


def _fmix32(h: torch.Tensor) -> torch.Tensor:
    """murmur3's 32-bit finaliser on int64 tensors holding 32-bit words."""
    h = h ^ (h >> 16)
    h = _mul32(h, 0x85EBCA6B)
    h = h ^ (h >> 13)
    h = _mul32(h, 0xC2B2AE35)
    return h ^ (h >> 16)


def uplink_key(seed: int, round_idx: int, rank: int) -> int:
    """The 64-bit key of one rank's draws in one round.  The rank enters
    because client ids are per-rank shards; the round, so that a resumed
    run draws what it would have drawn."""
    return (seed * 1_000_003 + round_idx * 7919 + rank * 2_654_435_761
            + 0xC0DEC) % (1 << 64)


def uplink_words(key: int, client_ids: torch.Tensor,
                 p: torch.Tensor) -> torch.Tensor:
    """The 32-bit hash word of every (client, element pair p) as int64
    [C, len(p)]: fmix32(ckey ^ (p * 0x9E3779B9)) with ckey =
    fmix32(fmix32(k0 ^ cid) ^ k1), (k0, k1) the low and high words of
    key.  client_ids and p are integer tensors of values below 2^32."""
    k0, k1 = key & _M32, (key >> 32) & _M32
    cid = client_ids.to(torch.int64).reshape(-1, 1)
    p = p.to(torch.int64).reshape(1, -1)
    ckey = _fmix32(_fmix32(cid ^ k0) ^ k1)
    return _fmix32(ckey ^ _mul32(p, 0x9E3779B9))


def uplink_uniform(key: int, client_ids: torch.Tensor,
                   j: torch.Tensor) -> torch.Tensor:
    """u in [0, 1) as fp32 [C, len(j)], a multiple of 2^-16: the uniform
    that client client_ids[c] draws for the element at index j of the flat
    master under key.  One hash word serves the pair (2p, 2p+1): the even
    element takes its low half, the odd one its high half."""
    j = j.to(torch.int64).reshape(-1)
    word = uplink_words(key, client_ids, j >> 1)
    half = torch.where((j & 1).reshape(1, -1) == 0, word & 0xFFFF, word >> 16)
    return half.to(torch.float32) / 65536.0


def uplink_bytes_per_client(numels: Sequence[int], bits: int) -> int:
    """Bytes one client's compressed update puts on the wire: the packed
    levels plus one fp32 scale per bucket, summed over parameter tensors."""
    uplink_levels(bits)
    return sum((n * bits + 7) // 8
               + 4 * ((n + UPLINK_BUCKET - 1) // UPLINK_BUCKET)
               for n in numels)


def _quantise_eager(diff: torch.Tensor, u: torch.Tensor,
                    levels: int) -> torch.Tensor:
    """Q of the contract for fp32 diff [C, n] and uniforms u [C, n]."""
    C, n = diff.shape
    pad = (-n) % UPLINK_BUCKET
    d = torch.nn.functional.pad(diff, (0, pad)).view(C, -1, UPLINK_BUCKET)
    a = d.abs().amax(dim=2, keepdim=True)
    L = float(levels)
    safe = torch.where(a == 0, torch.ones_like(a), a)
    t = d.abs() * L / safe
    fl = t.floor()
    up = torch.nn.functional.pad(u, (0, pad)).view_as(d)
    lvl = torch.minimum(fl + (up < t - fl).float(), torch.full_like(t, L))
    q = torch.sign(d) * lvl * (a / L)
    return q.view(C, -1)[:, :n]


def weighted_delta_accum_quant(delta: Sequence[torch.Tensor],
                               client_params: Sequence[torch.Tensor],
                               global_params: Sequence[torch.Tensor],
                               weights: torch.Tensor,
                               client_ids: torch.Tensor, bits: int, key: int,
                               elem_offsets: Sequence[int]) -> None:
    """delta[i] (fp32) += sum_c weights[c] * Q(client_params[i][c] -
    global_params[i]): weighted_delta_accum over updates quantised to
    `bits` bits per weight (2, 4 or 8; the rule above).

    client_ids [C] int64: the clients' ids; key: uplink_key's 64-bit
    value; elem_offsets[i]: where global_params[i] starts in the flat
    master.  Ids and pair indices are hashed as 32-bit words: every id and
    every (elem_offsets[i] + numel) / 2 must be below 2^32.

    GPU: one launch per parameter (csrc/uplink_quant.hip), deterministic
    below 64 clients.  CPU: the same rule in fp32 torch ops."""
    levels = uplink_levels(bits)
    if not delta:
        return
    key = int(key) % (1 << 64)
    for off, gw in zip(elem_offsets, global_params):
        if off < 0 or off + gw.numel() > (1 << 33):
            raise ValueError("uplink quantiser: element index "
                             f"{off + gw.numel()} past 2^33")
    if client_params[0].is_cuda:
        ops = load_hip_ops(required=True)
        C = client_params[0].shape[0]
        w = weights.float().contiguous()
        cid = client_ids.to(torch.int64).contiguous()
        # one host read for all the launches
        lo, hi = (int(x) for x in torch.aminmax(cid))
        if lo < 0 or hi > _M32:
            raise ValueError("uplink quantiser: client ids must lie in "
                             "0..2^32-1")
        for dl, cw, gw, off in zip(delta, client_params, global_params,
                                   elem_offsets):
            ops.delta_accum_quant(dl.reshape(-1), cw.detach().reshape(-1),
                                  gw.detach().reshape(-1), w, cid, C,
                                  int(bits), key & _M32, (key >> 32) & _M32,
                                  int(off), True)
        return
    with torch.no_grad():
        ids = client_ids.to(torch.int64).cpu()
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) > _M32):
            raise ValueError("uplink quantiser: client ids must lie in "
                             "0..2^32-1")
        C = ids.numel()
        w = weights.float().view(C, 1)
        for dl, cw, gw, off in zip(delta, client_params, global_params,
                                   elem_offsets):
            n = gw.numel()
            diff = cw.float().reshape(C, n) - gw.float().reshape(1, n)
            u = uplink_uniform(key, ids, off + torch.arange(n))
            q = _quantise_eager(diff, u, levels)
            dl.reshape(-1).add_((q * w).sum(dim=0))


def apply_aggregate(global_params: Sequence[torch.Tensor],
                    delta: Sequence[torch.Tensor],
                    total_weight: float) -> None:
    """w_global += delta / total_weight, in place (fp32 master weights)."""
    if total_weight == 0:
        return
    with torch.no_grad():
        inv = 1.0 / float(total_weight)
        torch._foreach_add_([g for g in global_params],
                            [d for d in delta], alpha=inv)


# -- server optimiser step --------------------------------------------------

SERVER_OPT_KINDS = ("momentum", "adagrad", "adam", "yogi")


def server_opt_step_eager(kind: str, master: torch.Tensor,
                          delta: torch.Tensor, m: torch.Tensor,
                          v: Optional[torch.Tensor], total_weight: float,
                          lr: float, beta1: float, beta2: float, tau: float,
                          noise: Optional[torch.Tensor] = None,
                          sigma: float = 0.0) -> None:
    """The rule of server_opt_step composed from torch ops on whatever
    device the tensors are on: the CPU path, and what the fused kernel is
    timed against (tools/serveroptbench.py)."""
    with torch.no_grad():
        g = delta * (1.0 / float(total_weight))
        if noise is not None:
            g.add_(noise, alpha=float(sigma))
        if kind == "momentum":
            m.mul_(beta1).add_(g)
            master.add_(m, alpha=lr)
            return
        m.mul_(beta1).add_(g, alpha=1.0 - beta1)
        g2 = g * g
        if kind == "adagrad":
            v.add_(g2)
        elif kind == "adam":
            v.mul_(beta2).add_(g2, alpha=1.0 - beta2)
        else:
            v.sub_(g2 * torch.sign(v - g2), alpha=1.0 - beta2)
        master.addcdiv_(m, v.sqrt().add_(tau), value=lr)


def server_opt_step(kind: str, master: torch.Tensor, delta: torch.Tensor,
                    m: torch.Tensor, v: Optional[torch.Tensor],
                    total_weight: float, lr: float, beta1: float,
                    beta2: float, tau: float,
                    noise: Optional[torch.Tensor] = None,
                    sigma: float = 0.0) -> None:
    """One server optimiser step on the flat fp32 master, in place.

    g = delta / total_weight + sigma * noise (noise None: no second term)

    - "momentum": m = beta1*m + g;              master += lr*m
    - "adagrad":  m = beta1*m + (1-beta1)*g;    v = v + g^2
    - "adam":     same m;        v = beta2*v + (1-beta2)*g^2
    - "yogi":     same m;        v = v - (1-beta2)*g^2*sign(v - g^2)
    - the three adaptive kinds: master += lr*m / (sqrt(v) + tau)

    No bias correction.  master, m and v (None or empty for "momentum")
    are updated; delta and noise are only read.  total_weight == 0 takes
    no step.  GPU: one launch (csrc/server_opt.hip)."""
    if kind not in SERVER_OPT_KINDS:
        raise ValueError(f"server optimiser {kind!r} not one of "
                         f"{SERVER_OPT_KINDS}")
    if total_weight == 0:
        return
    if master.is_cuda:
        ops = load_hip_ops(required=True)
        if v is None:
            v = torch.empty(0, dtype=master.dtype, device=master.device)
        ops.server_opt_step(SERVER_OPT_KINDS.index(kind), master, delta, m,
                            v, noise, float(total_weight), float(sigma),
                            float(lr), float(beta1), float(beta2),
                            float(tau))
        return
    server_opt_step_eager(kind, master, delta, m, v, total_weight, lr, beta1,
                          beta2, tau, noise, sigma)


# -- flat (single-buffer) forms used by the engine hot path ----------------
#
# Replica layout (engine/client_manager.replicate_flat): the 1-D buffer of
# length C*P is the concatenation over parameter blocks of [C, n_b]; block
# b covers global-master elements offsets[b]:offsets[b+1].

def fused_sgd_update_flat(buf: torch.Tensor, grad: torch.Tensor,
                          global_flat: torch.Tensor, clients: int,
                          lr: float, mu: float,
                          offsets: Optional[torch.Tensor] = None) -> None:
    """buf -= lr * (grad + mu * (buf - replicated(global_flat))), in place."""
    if buf.is_cuda:
        ops = load_hip_ops(required=True)
        ops.fused_sgd_update_flat(
            buf, grad,
            global_flat if mu != 0.0 else torch.empty(0, dtype=buf.dtype, device=buf.device),
            offsets if (mu != 0.0 and offsets is not None) else
            torch.empty(0, dtype=torch.int64, device=buf.device),
            int(clients), float(lr), float(mu))
        return
    with torch.no_grad():
        if mu == 0.0 or offsets is None:
            buf.add_(grad, alpha=-lr)
            return
        offs = offsets.tolist()
        for b in range(len(offs) - 1):
            g0, g1 = offs[b], offs[b + 1]
            n = g1 - g0
            blk = buf[clients * g0:clients * g1].view(clients, n)
            gblk = grad[clients * g0:clients * g1].view(clients, n)
            prox = blk - global_flat[g0:g1].unsqueeze(0)
            blk.add_(gblk + mu * prox, alpha=-lr)


def weighted_delta_accum_flat(delta: torch.Tensor, buf: torch.Tensor,
                              global_flat: torch.Tensor,
                              weights: torch.Tensor, clients: int,
                              offsets: Optional[torch.Tensor] = None,
                              wsum: Union[float, torch.Tensor, None] = None
                              ) -> None:
    """delta[j] += sum_c weights[c] * (buf[c,j] - global_flat[j]) per block.
    wsum: host float or one-element fp32 device tensor (see
    weighted_delta_accum)."""
    if buf.is_cuda:
        ops = load_hip_ops(required=True)
        if isinstance(wsum, torch.Tensor):
            ops.weighted_delta_accum_flat_dw(delta, buf, global_flat,
                                             weights.float(), offsets,
                                             int(clients), wsum)
            return
        if wsum is None:
            wsum = float(weights.sum())
        ops.weighted_delta_accum_flat(delta, buf, global_flat,
                                      weights.float(), offsets, int(clients),
                                      float(wsum))
        return
    with torch.no_grad():
        offs = offsets.tolist()
        w = weights.float().view(clients, 1)
        for b in range(len(offs) - 1):
            g0, g1 = offs[b], offs[b + 1]
            n = g1 - g0
            blk = buf[clients * g0:clients * g1].view(clients, n).float()
            diff = blk - global_flat[g0:g1].float().unsqueeze(0)
            delta[g0:g1].add_((diff * w).sum(dim=0))


class _CrossEntropyFn(torch.autograd.Function):
    """Fused CE over [N, K] logits (HIP kernel fwd computes loss AND
    dlogits in one pass; backward is a scale)."""

    @staticmethod
    def forward(ctx, logits: torch.Tensor, labels: torch.Tensor):
        ops = load_hip_ops(required=True)
        row_loss, dlogits = ops.cross_entropy_fwd_bwd(
            logits.contiguous(), labels)
        ctx.save_for_backward(dlogits)
        return row_loss.mean()

    @staticmethod
    def backward(ctx, grad_out):
        (dlogits,) = ctx.saved_tensors
        return dlogits * grad_out, None


def cross_entropy_fwd_bwd(logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """Mean cross-entropy over all rows. logits [N, K] (bf16/f32), labels [N] int64."""
    if logits.is_cuda:
        return _CrossEntropyFn.apply(logits, labels)
    return torch.nn.functional.cross_entropy(logits.float(), labels)


class _GroupNormActFn(torch.autograd.Function):
    """Fused per-client GroupNorm (+residual +ReLU) on channel-grouped
    activations [B, C*ch, H, W] (ops/csrc/groupnorm.hip)."""

    @staticmethod
    def forward(ctx, x, res, gamma, beta, clients, groups, eps, relu):
        ops = load_hip_ops(required=True)
        has_res = res is not None
        res_in = res.contiguous() if has_res else torch.empty(0, dtype=x.dtype,
                                                              device=x.device)
        y, mean, rstd = ops.groupnorm_fwd(x.contiguous(), res_in, gamma,
                                          beta, clients, groups, eps, relu)
        ctx.save_for_backward(x, y, mean, rstd, gamma)
        ctx.meta = (clients, groups, has_res, relu)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, mean, rstd, gamma = ctx.saved_tensors
        clients, groups, has_res, relu = ctx.meta
        ops = load_hip_ops(required=True)
        dx, dres, dgamma, dbeta = ops.groupnorm_bwd(
            x, y, dy, mean, rstd, gamma, clients, groups, has_res, relu)
        return (dx, dres.view_as(x) if has_res else None,
                dgamma.to(gamma.dtype), dbeta.to(gamma.dtype),
                None, None, None, None)


def groupnorm_act(x: torch.Tensor, clients: int, groups: int,
                  gamma: torch.Tensor, beta: torch.Tensor,
                  res: Optional[torch.Tensor] = None, relu: bool = False,
                  eps: float = 1e-5) -> torch.Tensor:
    """y = relu?(gn(x; clients, groups)*gamma + beta [+ res]).

    x 4-D [B, C*ch, H, W] (channel-grouped) or 5-D [C, ch, B, H, W]
    (client-channel-first, the conv-kernel layout).  GPU: one fused HIP
    kernel each way.  CPU: composed torch ops."""
    if x.is_cuda:
        return _GroupNormActFn.apply(x, res, gamma.contiguous(),
                                     beta.contiguous(), clients, groups,
                                     eps, relu)
    if x.dim() == 5:
        C, ch, B, H, W = x.shape
        cg = ch // groups
        xg = x.view(C, groups, cg, B, H, W)
        mean = xg.mean(dim=(2, 4, 5), keepdim=True)
        var = xg.var(dim=(2, 4, 5), unbiased=False, keepdim=True)
        y = ((xg - mean) * torch.rsqrt(var + eps)).view(C, ch, B, H, W)
        y = y * gamma.view(C, ch, 1, 1, 1) + beta.view(C, ch, 1, 1, 1)
    else:
        from ..models.base import bgroupnorm
        y = bgroupnorm(x, clients, groups, gamma, beta, eps)
    if res is not None:
        y = y + res
    return torch.nn.functional.relu(y) if relu else y


# -- padded-output GroupNorm (feeds the v6 padded 3x3 conv family) ----------
#
# A "padded pair" is (y, y_pad): y_pad is the activation [C, ch, B, H+2,
# W+2] with a 1-element zero halo that the kernels read; y is its interior
# view y_pad[..., 1:-1, 1:-1] and exists for the autograd graph only —
# gradients flow through it dense and unpadded, no kernel reads it.

def gn_pad_shape_ok(ch: int, groups: int, H: int, W: int) -> bool:
    """True when both LDS-staged directions of the padded pair fit a
    [*, ch, *, H, W] bf16 GPU activation and OLSIM_GN_PAD=0 (the A/B
    switch back to dense GN + pad2d) is not set."""
    if os.environ.get("OLSIM_GN_PAD", "1") == "0":
        return False
    ops = load_hip_ops(required=True)
    return bool(ops.gn_pad_ok(ch, groups, H, W))


def gn_pad_eligible(x: torch.Tensor, groups: int) -> bool:
    if not (x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 5):
        return False
    return gn_pad_shape_ok(x.shape[1], groups, x.shape[3], x.shape[4])


def _res_arg(x, res, res_pad):
    """Residual tensor handed to groupnorm_fwd_pad: the padded image when
    the residual is a padded pair, the dense tensor otherwise."""
    if res is None:
        return torch.empty(0, dtype=x.dtype, device=x.device)
    return res_pad if res_pad is not None else res.contiguous()


def _interior(y_pad: torch.Tensor) -> torch.Tensor:
    return y_pad[..., 1:-1, 1:-1]


class _GroupNormPadFn(torch.autograd.Function):
    """relu(gn(x) [+ res]) written as a padded pair.  Saves x and a 1-bit
    ReLU mask (not y) for the backward."""

    @staticmethod
    def forward(ctx, x, res, res_pad, gamma, beta, clients, groups, eps):
        ops = load_hip_ops(required=True)
        y_pad, mask, mean, rstd = ops.groupnorm_fwd_pad(
            x, _res_arg(x, res, res_pad), gamma, beta, clients, groups, eps,
            True)
        ctx.save_for_backward(x, mask, mean, rstd, gamma)
        ctx.meta = (clients, groups, res is not None)
        ctx.mark_non_differentiable(y_pad)
        # y_pad never has a gradient; do not let autograd zero-fill one
        ctx.set_materialize_grads(False)
        return _interior(y_pad), y_pad

    @staticmethod
    def backward(ctx, dy, _dy_pad):
        x, mask, mean, rstd, gamma = ctx.saved_tensors
        clients, groups, has_res = ctx.meta
        if dy is None:
            return (None,) * 8
        ops = load_hip_ops(required=True)
        dx, _, dres, dgamma, dbeta = ops.groupnorm_bwd_pad(
            x, mask, dy, mean, rstd, gamma, clients, groups, has_res, False)
        return (dx, dres if has_res else None, None,
                dgamma.to(gamma.dtype), dbeta.to(gamma.dtype),
                None, None, None)


def groupnorm_relu_pad(x: torch.Tensor, clients: int, groups: int,
                       gamma: torch.Tensor, beta: torch.Tensor,
                       res: Optional[torch.Tensor] = None,
                       res_pad: Optional[torch.Tensor] = None,
                       eps: float = 1e-5):
    """relu(gn(x)*gamma + beta [+ res]) for x [C, ch, B, H, W] as a padded
    pair (y, y_pad).  res may itself be a padded pair (res, res_pad).
    Ineligible shapes take the dense kernels and return (y, None); the
    consuming conv then pads its input itself."""
    if gn_pad_eligible(x, groups):
        return _GroupNormPadFn.apply(x.contiguous(), res, res_pad,
                                     gamma.contiguous(), beta.contiguous(),
                                     clients, groups, eps)
    return groupnorm_act(x, clients, groups, gamma, beta, res=res,
                         relu=True, eps=eps), None


def fast_transpose(x: torch.Tensor) -> torch.Tensor:
    """[B, M, N] -> contiguous [B, N, M] via the LDS-tiled transpose
    kernel (torch's transpose+contiguous runs the generic strided copy
    at a fraction of the roofline on large batched matrices).  The
    kernels put the batch on grid.z, so a batch past 65535 goes to torch."""
    if x.is_cuda and x.dim() == 3 and x.shape[0] <= 65535 and \
            x.dtype in (torch.bfloat16, torch.float32):
        ops = load_hip_ops()
        if ops is not None:
            return ops.transpose2d(x.contiguous())
    return x.transpose(1, 2).contiguous()


class _LayerNormFn(torch.autograd.Function):
    """Fused per-client LayerNorm over the trailing dim
    (ops/csrc/layernorm.hip; one wave per row, fp32 dgamma/dbeta
    partials through workgroup LDS)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        ops = load_hip_ops(required=True)
        y, mean, rstd = ops.layernorm_fwd(x, gamma, beta, eps)
        ctx.save_for_backward(x, gamma, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, gamma, mean, rstd = ctx.saved_tensors
        ops = load_hip_ops(required=True)
        dx, dgamma, dbeta = ops.layernorm_bwd(x, dy.contiguous(), gamma,
                                              mean, rstd)
        return dx, dgamma.to(gamma.dtype), dbeta.to(gamma.dtype), None


def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor,
              eps: float = 1e-5):
    """Per-client LayerNorm: x [C, ..., H], gamma/beta [C, H].
    Fused kernel on GPU when H%8==0 and rows-per-client %4==0;
    None -> caller should use the composed fallback."""
    shape = x.shape
    C, H = shape[0], shape[-1]
    n = x.numel() // (C * H)
    if not (x.is_cuda and H % 8 == 0 and n % 4 == 0 and H <= 1536
            and x.dtype in (torch.bfloat16, torch.float32)
            and hip_ops_available()):
        return None
    y = _LayerNormFn.apply(x.reshape(C, n, H).contiguous(), gamma, beta, eps)
    return y.view(shape)
