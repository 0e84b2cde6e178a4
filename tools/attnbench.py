"""Fused causal attention against the library route, in one process.

At the benchmark's shape (C 125, B 4, L 128, 12 heads of 64, bf16): one
attention layer forward + backward, from the output of the qkv blinear to
the gradient of that output, so the torch route is timed with its permutes,
the transpose copy of the output and the assembly of dqkv.  Both routes
alternate after warm-up, device events over windows of at least a second.
Prints one JSON line: ms per route as the median over the repeats with
their min..max spread, the kernel launches of one step (counted by the
profiler), and the fused kernels' useful bytes/s and FLOP/s from the shapes.

--seq-len L (default 128) times another length at the same 512 tokens per
client (B = 512 // L): from 129 on the "fused" side is the long-sequence
kernels of attn_long.hip.

    python tools/attnbench.py [--clients 125] [--repeats 5] [--seq-len 128]
"""

import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from olearning_sim_amd.ops import attn                    # noqa: E402

B, L, HEADS, HD = 4, 128, 12, 64
H = HEADS * HD


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
    qkv = torch.randn(C, B * L, 3 * H, device="cuda", generator=gen) \
        .bfloat16().requires_grad_(True)
    datt = torch.randn(C, B * L, H, device="cuda", generator=gen).bfloat16()

    def step():
        x = qkv.view(C, B, L, 3 * H)
        if attn.attn_route(x, HEADS) == "fused":
            att = attn.causal_attention(x, HEADS).view(C, B * L, H)
        elif attn.attn_long_route(x, HEADS) == "long":
            att = attn.causal_attention_long(x, HEADS).view(C, B * L, H)
        else:       # the lines of models/bert.py::encode
            x = qkv.view(C * B, L, 3, HEADS, HD).permute(2, 0, 3, 1, 4)
            att = F.scaled_dot_product_attention(x[0], x[1], x[2],
                                                 is_causal=True)
            att = att.transpose(1, 2).reshape(C, B * L, H)
        torch.autograd.grad(att, qkv, datt)
    return step


def useful(C):
    """(bytes, FLOP) one forward + backward needs, from the shapes: every
    operand once per kernel that takes it (forward qkv, att, lse; backward
    qkv, att, datt, lse, dqkv), and the causal half, diagonal included, of
    the 2 forward and 5 backward products, each counted once (the kernel
    computes S and dP in both of its backward phases).  The long kernels
    add the row-dot pass: att and datt read, D written and read."""
    rows = C * B * L
    nbytes = rows * H * 2 * (3 + 1 + 3 + 1 + 1 + 3) + 2 * rows * HEADS * 4
    if L > 128:
        nbytes += rows * H * 2 * 2 + 2 * rows * HEADS * 4
    pairs = C * B * HEADS * L * (L + 1) // 2
    return nbytes, 2 * HD * pairs * (2 + 5)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, default=125)
    ap.add_argument("--repeats", type=int, default=5)
    global B, L
    ap.add_argument("--seq-len", type=int, default=L)
    args = ap.parse_args()
    L = args.seq_len
    B = max(1, 512 // L)
    C = args.clients
    step = layer_step(C)
    res = {"fused": [], "torch": []}
    count = {}
    for route in res:
        os.environ["OLSIM_ATTN"] = route
        for _ in range(3):
            step()
        count[route] = launches(step)
    for _ in range(args.repeats):
        for route in res:
            os.environ["OLSIM_ATTN"] = route
            res[route].append(window_ms(step))
    out = {"C": C, "B": B, "L": L, "heads": HEADS, "HD": HD}
    for route, ms in res.items():
        out[route + "_ms"] = round(statistics.median(ms), 4)
        out[route + "_spread_ms"] = [round(min(ms), 4), round(max(ms), 4)]
        out[route + "_launches"] = count[route]
    out["speedup"] = round(out["torch_ms"] / out["fused_ms"], 3)
    nbytes, flop = useful(C)
    out["fused_useful_GBps"] = round(nbytes / out["fused_ms"] / 1e6, 1)
    out["fused_TFLOPs"] = round(flop / out["fused_ms"] / 1e9, 2)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
