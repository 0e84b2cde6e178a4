"""The tied head's fused cross-entropy against the library route, in one
process.

At the benchmark's shape (C 125, N 512, H 768, V 30522, bf16): tied_head_ce
forward + backward from the hidden states to their gradient, the GEMMs of
both routes included.  Both routes alternate after warm-up, device events
over windows of at least a second.  Prints one JSON line: ms per route as
the median over the repeats with their min..max spread, the kernel launches
of one step (counted by the profiler), the peak of allocated memory per
route, and for each VEC variant that shape reaches (the full slices at 8,
the tail at 2) the two kernels' own time on one tile and their useful
bytes/s from the shapes.

    python tools/headcebench.py [--clients 125] [--repeats 5]
"""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from olearning_sim_amd.models.bert import _TiedHeadCE, tied_head_ce  # noqa: E402
from olearning_sim_amd.ops import head_ce                  # noqa: E402

N, H, V = 512, 768, 30522


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


def head_step(C):
    gen = torch.Generator(device="cuda").manual_seed(0)
    hs = torch.randn(C, N, H, device="cuda", generator=gen).bfloat16() \
        .requires_grad_(True)
    tok = (0.02 * torch.randn(C, V, H, device="cuda", generator=gen)) \
        .bfloat16().requires_grad_(True)
    bias = torch.zeros(V, device="cuda", dtype=torch.bfloat16) \
        .requires_grad_(True)
    labels = torch.randint(0, V, (C, N), device="cuda", generator=gen)

    def step():       # the head's lines of models/bert.py::BertLM.loss
        loss = tied_head_ce(hs, tok, bias.unsqueeze(0).expand(C, -1), labels)
        torch.autograd.grad(loss, (hs, tok, bias))
    return step


def kernels(C, s, s0, min_s=0.3):
    """ms and useful GB/s of each kernel on one [C, N, s] tile: the tile
    once per kernel that reads or writes it plus the per-row operands."""
    gen = torch.Generator(device="cuda").manual_seed(s)
    tile = torch.randn(C, N, s, device="cuda", generator=gen).bfloat16()
    bias = torch.zeros(C, V, device="cuda", dtype=torch.bfloat16)
    labels = torch.randint(0, V, (C, N), device="cuda", generator=gen)
    m = torch.full((C, N), float("-inf"), device="cuda")
    l, zy = torch.zeros_like(m), torch.zeros_like(m)
    g = torch.full((1,), 1.0 / (C * N), device="cuda")
    dbias, out = torch.empty_like(bias), torch.empty_like(tile)
    head_ce.head_ce_stats(tile, bias, labels, s0, m, l, zy)
    ms_s = window_ms(lambda: head_ce.head_ce_stats(tile, bias, labels, s0, m,
                                                   l, zy), min_s)
    ms_g = window_ms(lambda: head_ce.head_ce_grad(tile, bias, labels, s0, m,
                                                  l, g, dbias, out), min_s)
    rows = C * N * (8 + 2 * 4)
    return {"route": head_ce.head_ce_route(tile), "s": s,
            "stats_ms": round(ms_s, 4), "grad_ms": round(ms_g, 4),
            "stats_useful_GBps": round((tile.numel() * 2 + rows + C * N * 12
                                        + C * s * 2) / ms_s / 1e6, 1),
            "grad_useful_GBps": round((tile.numel() * 4 + rows + C * s * 4)
                                      / ms_g / 1e6, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, default=125)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    C = args.clients
    step = head_step(C)
    res = {"fused": [], "torch": []}
    count, peak = {}, {}
    for route in res:
        os.environ["OLSIM_HEAD_CE"] = route
        for _ in range(3):
            step()
        count[route] = launches(step)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        step()
        torch.cuda.synchronize()
        peak[route] = torch.cuda.max_memory_allocated()
    for _ in range(args.repeats):
        for route in res:
            os.environ["OLSIM_HEAD_CE"] = route
            res[route].append(window_ms(step))
    os.environ["OLSIM_HEAD_CE"] = "fused"
    out = {"C": C, "N": N, "H": H, "V": V, "slice": _TiedHeadCE.SLICE_V}
    for route, ms in res.items():
        out[route + "_ms"] = round(statistics.median(ms), 4)
        out[route + "_spread_ms"] = [round(min(ms), 4), round(max(ms), 4)]
        out[route + "_launches"] = count[route]
        out[route + "_peak_GB"] = round(peak[route] / 1e9, 3)
    out["speedup"] = round(out["torch_ms"] / out["fused_ms"], 3)
    sv = _TiedHeadCE.SLICE_V
    out["kernels"] = [kernels(C, sv, 0), kernels(C, V % sv, V - V % sv)]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
