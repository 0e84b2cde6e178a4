"""Fused LSTM recurrence against the torch loop, in one process.

At the workload shape (B 16, L 80, H 256, 2 layers, bf16) and C in
{256, 1024}: one layer's forward + backward, and a whole CharLSTM
model.loss + autograd.grad step, on the fused route and under
OLSIM_LSTM=torch, alternating after warm-up, device events over windows
of at least a second.  Prints one JSON line per (C, what): ms per route
as the median over the repeats with their min..max spread, the kernel
launches of one step (counted by the profiler), and the fused kernels'
useful bytes/s.

    python tools/lstmbench.py [--clients 256 1024] [--repeats 5]
"""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from olearning_sim_amd.models import build_model          # noqa: E402
from olearning_sim_amd.models.base import blinear         # noqa: E402
from olearning_sim_amd.ops import lstm                    # noqa: E402

B, L, H, LAYERS, V = 16, 80, 256, 2, 90


def set_route(route):
    os.environ["OLSIM_LSTM"] = route


def window_ms(fn, min_s=1.0):
    """ms per call of fn over one window of at least min_s seconds."""
    n = 1
    while True:
        start, stop = (torch.cuda.Event(enable_timing=True) for _ in "ab")
        start.record()
        for _ in range(n):
            fn()
        stop.record()
        stop.synchronize()
        ms = start.elapsed_time(stop)
        if ms >= 1000.0 * min_s:
            return ms / n
        n = max(n + 1, int(n * 1200.0 * min_s / max(ms, 1e-3)))


def launches(fn):
    fn()
    torch.cuda.synchronize()
    with torch.profiler.profile(
            activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(e.count for e in prof.key_averages()
               if e.device_type == torch.autograd.DeviceType.CUDA)


def layer_step(C):
    gen = torch.Generator(device="cuda").manual_seed(0)
    xp = torch.randn(C, B, L, 4 * H, device="cuda", generator=gen) \
        .bfloat16().requires_grad_(True)
    w = (torch.randn(C, H, 4 * H, device="cuda", generator=gen) / 16) \
        .bfloat16().requires_grad_(True)
    dhs = torch.randn(C, B, L, H, device="cuda", generator=gen).bfloat16()

    def torch_layer():
        ht = torch.zeros(C, B, H, device="cuda", dtype=torch.bfloat16)
        ct, outs = torch.zeros_like(ht), []
        for t in range(L):
            i, f, g, o = (xp[:, :, t] + blinear(ht, w)).split(H, dim=-1)
            ct = torch.sigmoid(f) * ct + torch.sigmoid(i) * torch.tanh(g)
            ht = torch.sigmoid(o) * torch.tanh(ct)
            outs.append(ht)
        return torch.stack(outs, dim=2)

    def step():
        fused = lstm.lstm_route(xp, w) == "fused"
        hs = lstm.lstm_layer(xp, w) if fused else torch_layer()
        torch.autograd.grad(hs, (xp, w), dhs)
    return step


def model_step(C):
    model = build_model("lstm", vocab_size=V, embed=8, hidden=H,
                        layers=LAYERS, seq_len=L)
    params = model.replicate(
        model.init_global("cuda", generator=torch.Generator("cuda")
                          .manual_seed(0)), C, torch.bfloat16)
    x = torch.randint(0, V, (C, B, L), device="cuda")
    y = torch.randint(0, V, (C, B, L), device="cuda")

    def step():
        torch.autograd.grad(model.loss(params, x, y), list(params.values()))
    return step


def fused_bytes(C, layers):
    """Useful bytes of the fused kernels per step: the weight stream of both
    directions (C*L*H*4H*2 each) plus every activation tensor once."""
    stream = 2 * C * L * H * 4 * H * 2
    acts_fwd = C * B * L * H * (4 * 2 + 4 * 2 + 2 + 4)     # xp gates hs cs
    acts_bwd = C * B * L * H * (2 + 4 * 2 + 2 * 4 + 4 * 2)  # dhs gates cs dgates
    return layers * (stream + acts_fwd + acts_bwd)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    for C in args.clients:
        for what, make, layers in (("layer", layer_step, 1),
                                   ("model", model_step, LAYERS)):
            step = make(C)
            res = {"fused": [], "torch": []}
            count = {}
            for route in res:
                set_route(route)
                for _ in range(3):
                    step()
                count[route] = launches(step)
            for _ in range(args.repeats):
                for route in res:
                    set_route(route)
                    res[route].append(window_ms(step))
            out = {"C": C, "what": what, "B": B, "L": L, "H": H}
            for route, ms in res.items():
                out[route + "_ms"] = round(statistics.median(ms), 3)
                out[route + "_spread_ms"] = [round(min(ms), 3),
                                             round(max(ms), 3)]
                out[route + "_launches"] = count[route]
            out["speedup"] = round(out["torch_ms"] / out["fused_ms"], 3)
            if what == "layer":
                out["fused_useful_GBps"] = round(
                    fused_bytes(C, layers) / out["fused_ms"] / 1e6, 1)
            print(json.dumps(out), flush=True)
            del step
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
