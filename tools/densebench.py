"""The fused dense-layer epilogues against the composed route, in one process.

At the benchmark's shape (C 125, N 512, H 768, bf16): the dense part of one
BertLM encoder layer, forward + backward: attn_out + residual + ln1, ffn_in +
GELU, ffn_out + residual + ln2, the GEMMs of both routes included.  Both
routes alternate after warm-up, device events over windows of at least a
second.  Prints one JSON line: ms per route as the median over the repeats
with their min..max spread, the kernel launches of one step (counted by the
profiler), each kernel's own time and useful bytes/s from the shapes, and the
two backward kernels at each candidate row block.

    python tools/densebench.py [--clients 125] [--repeats 5]
"""

import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from olearning_sim_amd.models.base import blayernorm, blinear  # noqa: E402
from olearning_sim_amd.models.bert import _dense_epi_fused      # noqa: E402
from olearning_sim_amd.ops import dense_epi                     # noqa: E402
from olearning_sim_amd.ops.dense_epi import (                   # noqa: E402
    bias_gelu, bias_residual_layernorm)

N, H = 512, 768
BF16 = torch.bfloat16


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

    def t(*shape, std=1.0, mean=0.0):
        return (mean + std * torch.randn(*shape, device="cuda", generator=gen)) \
            .to(BF16).requires_grad_(True)

    p = {"l0.attn_out.w": t(C, H, H, std=0.03), "l0.attn_out.b": t(C, H),
         "l0.ln1.g": t(C, H, std=0.1, mean=1.0), "l0.ln1.b": t(C, H, std=0.1),
         "l0.ffn_in.w": t(C, H, 4 * H, std=0.03), "l0.ffn_in.b": t(C, 4 * H),
         "l0.ffn_out.w": t(C, 4 * H, H, std=0.02), "l0.ffn_out.b": t(C, H),
         "l0.ln2.g": t(C, H, std=0.1, mean=1.0), "l0.ln2.b": t(C, H, std=0.1)}
    hs0, att = t(C, N, H), t(C, N, H)
    dy = torch.randn(C, N, H, device="cuda", generator=gen).to(BF16)

    def step():       # the dense lines of models/bert.py::BertLM.encode
        if _dense_epi_fused(hs0, p, "l0"):
            hs = bias_residual_layernorm(
                blinear(att, p["l0.attn_out.w"], None), p["l0.attn_out.b"],
                hs0, p["l0.ln1.g"], p["l0.ln1.b"])
            ff = bias_gelu(blinear(hs, p["l0.ffn_in.w"], None),
                           p["l0.ffn_in.b"])
            hs = bias_residual_layernorm(
                blinear(ff, p["l0.ffn_out.w"], None), p["l0.ffn_out.b"], hs,
                p["l0.ln2.g"], p["l0.ln2.b"])
        else:
            hs = hs0 + blinear(att, p["l0.attn_out.w"], p["l0.attn_out.b"])
            hs = blayernorm(hs, p["l0.ln1.g"], p["l0.ln1.b"])
            ff = F.gelu(blinear(hs, p["l0.ffn_in.w"], p["l0.ffn_in.b"]))
            hs = hs + blinear(ff, p["l0.ffn_out.w"], p["l0.ffn_out.b"])
            hs = blayernorm(hs, p["l0.ln2.g"], p["l0.ln2.b"])
        torch.autograd.grad(hs, [hs0, att] + list(p.values()), dy)
    return step


def kernels(C, min_s=0.3):
    """ms and useful GB/s of each kernel (the finish included in the
    backwards): every row tensor once per read or write, from the shapes."""
    gen = torch.Generator(device="cuda").manual_seed(1)

    def t(*shape):
        return torch.randn(*shape, device="cuda", generator=gen).to(BF16)

    out = {}
    unit = C * N * H * 2                      # one [C, N, H] bf16 tensor
    z, b, dy = t(C, N, 4 * H), t(C, 4 * H), t(C, N, 4 * H)
    y, dz = torch.empty_like(z), torch.empty_like(z)
    ms = window_ms(lambda: dense_epi.bias_gelu_fwd(z, b, out=y), min_s)
    out["bias_gelu_fwd"] = {"ms": round(ms, 4),
                            "useful_GBps": round(8 * unit / ms / 1e6, 1)}
    rows = {}
    for rb in (16, 32, 64):
        dense_epi.GELU_ROWS = rb
        ms = window_ms(lambda: dense_epi.bias_gelu_bwd(z, b, dy, dz=dz), min_s)
        rows[rb] = {"ms": round(ms, 4),
                    "useful_GBps": round(12 * unit / ms / 1e6, 1)}
    out["bias_gelu_bwd_by_rows"] = rows
    del z, dy, y, dz
    z, res, dy = t(C, N, H), t(C, N, H), t(C, N, H)
    b, g, be = t(C, H), t(C, H), t(C, H)
    y, s, mean, rstd = dense_epi.brln_fwd(z, b, res, g, be, 1e-5)
    ds = torch.empty_like(z)
    ms = window_ms(lambda: dense_epi.brln_fwd(z, b, res, g, be, 1e-5, y=y, s=s,
                                              mean=mean, rstd=rstd), min_s)
    out["brln_fwd"] = {"ms": round(ms, 4),
                       "useful_GBps": round(4 * unit / ms / 1e6, 1)}
    rows = {}
    for rb in (8, 16, 32, 64):
        dense_epi.LN_ROWS = rb
        ms = window_ms(lambda: dense_epi.brln_bwd(s, dy, g, mean, rstd, ds=ds),
                       min_s)
        rows[rb] = {"ms": round(ms, 4),
                    "useful_GBps": round(3 * unit / ms / 1e6, 1)}
    out["brln_bwd_by_rows"] = rows
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clients", type=int, default=125)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    C = args.clients
    gelu_rows, ln_rows = dense_epi.GELU_ROWS, dense_epi.LN_ROWS
    step = layer_step(C)
    res = {"fused": [], "torch": []}
    count = {}
    for route in res:
        os.environ["OLSIM_DENSE_EPI"] = route
        for _ in range(3):
            step()
        count[route] = launches(step)
    for _ in range(args.repeats):
        for route in res:
            os.environ["OLSIM_DENSE_EPI"] = route
            res[route].append(window_ms(step))
    os.environ["OLSIM_DENSE_EPI"] = "fused"
    out = {"C": C, "N": N, "H": H, "gelu_rows": gelu_rows, "ln_rows": ln_rows}
    for route, ms in res.items():
        out[route + "_ms"] = round(statistics.median(ms), 4)
        out[route + "_spread_ms"] = [round(min(ms), 4), round(max(ms), 4)]
        out[route + "_launches"] = count[route]
    out["speedup"] = round(out["torch_ms"] / out["fused_ms"], 3)
    out["kernels"] = kernels(C)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
