#!/usr/bin/env python3
"""Compare two builds of groupnorm.hip kernel by kernel.

    hipcc --offload-arch=gfx950 -O3 --offload-device-only -S \\
        olearning_sim_amd/ops/csrc/groupnorm.hip -o new.s     # and old.s
    python tools/gn_fp_histogram.py old.s new.s

For every kernel the two files have in common it counts the instructions
that decide the results and the memory traffic (floating-point ALU,
conversions, atomics, LDS and vector memory, barriers) and prints the
kernels whose counts differ.  Equal counts mean the same arithmetic in a
possibly different schedule; a changed v_fma/v_fmac/v_pk_* count means a
product is fused or packed differently and the output bits may move.
Exit status 1 if any kernel differs.  See docs/KERNEL_NOTES.md,
"GroupNorm: shared pieces".
"""
import collections
import re
import sys

WATCHED = re.compile(r"_f32|_f16|_bf16|_f64|rsq|rcp|sqrt|atomic|ds_add|"
                     r"ds_pk_add|ds_bpermute|ds_swizzle|dpp|permlane|"
                     r"global_store|global_load_dwordx|ds_read_b(64|128)|"
                     r"ds_write_b(64|128)|s_barrier")


def kernels(path):
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = m.group(1)
            out[cur] = collections.Counter()
            continue
        m = re.match(r"^\s+([a-z_0-9]+)(\s|$)", line)
        if cur and m:
            if WATCHED.search(m.group(1)):
                out[cur][m.group(1)] += 1
            if m.group(1) == "s_endpgm":
                cur = None
    return out


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    common = sorted(set(old) & set(new))
    differ = 0
    for k in common:
        if old[k] != new[k]:
            differ += 1
            ops = sorted(set(old[k]) | set(new[k]))
            print(k, {o: (old[k][o], new[k][o]) for o in ops
                      if old[k][o] != new[k][o]})
    print(f"{len(common) - differ} of {len(common)} kernels identical "
          f"({len(set(old) ^ set(new))} present in one file only)")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
