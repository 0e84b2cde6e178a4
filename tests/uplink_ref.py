"""The uplink quantiser's contract in numpy, with none of the package's
code: the counter hash on Python-int / uint64 arithmetic, the bucketed
stochastic quantiser in fp64, and the element-wise checks that the CPU
path (test_uplink_quant_cpu.py) and the HIP kernels
(test_uplink_quant_gpu.py) are both held to.

    d = f32(buf) - f32(master)   in fp32, per element
    a = max |d| over the bucket of 512 elements of the tensor
    t = |d| * L / a,  L = 2^(bits-1) - 1
    l = min(L, floor(t) + [u < t - floor(t)])
    Q = sign(d) * l * (a / L),  Q = 0 where a == 0

A kernel evaluates t in fp32, off from t64 by at most 3 * 2^-24 * 127 =
2.3e-5, so where frac(t64) lies within 2^-14 of u it may choose the other
neighbour: the *ambiguous set*.  Its expected share is 2 * 2^-14 = 1.2e-4.
"""

import numpy as np
import torch

BUCKET = 512
AMBIGUOUS = 2.0 ** -14
M32 = 0xFFFFFFFF
# a large even element offset: the pair index of its elements needs all
# 32 bits
BIG_BASE = 2 ** 32 + 2 ** 31 + 4096

HASH_VECTORS = [  # (k0, k1, cid, p, word)
    (1, 0, 0, 0, 0x5716F995),
    (0x1234ABCD, 0x0BADF00D, 5, 3, 0xCE608EDC),
    (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0x71F0E19A),
    (7, 9, 1249, 5600000, 0x267E1F09),
]


def levels(bits):
    return {2: 1, 4: 7, 8: 127}[bits]


def fmix32(h):
    h = np.asarray(h, dtype=np.uint64) & np.uint64(M32)
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85EBCA6B)) & np.uint64(M32)
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xC2B2AE35)) & np.uint64(M32)
    return h ^ (h >> np.uint64(16))


def words(key, cids, p):
    """uint64 [C, len(p)] of 32-bit words."""
    k0, k1 = np.uint64(key & M32), np.uint64((key >> 32) & M32)
    cid = np.asarray(cids, dtype=np.uint64).reshape(-1, 1)
    p = np.asarray(p, dtype=np.uint64).reshape(1, -1)
    ckey = fmix32(fmix32(cid ^ k0) ^ k1)
    return fmix32(ckey ^ ((p * np.uint64(0x9E3779B9)) & np.uint64(M32)))


def uniform(key, cids, j):
    """fp64 [C, len(j)]: u of client cids[c] at flat-master index j."""
    j = np.asarray(j, dtype=np.uint64).reshape(-1)
    w = words(key, cids, j >> np.uint64(1))
    half = np.where((j & np.uint64(1)).reshape(1, -1) == 0,
                    w & np.uint64(0xFFFF), w >> np.uint64(16))
    return half.astype(np.float64) / 65536.0


def key_of(seed, round_idx, rank):
    return (seed * 1_000_003 + round_idx * 7919 + rank * 2_654_435_761
            + 0xC0DEC) % (1 << 64)


def bytes_per_client(numels, bits):
    return sum(-(-n * bits // 8) + 4 * -(-n // BUCKET) for n in numels)


def quantise(buf, master, key, cids, elem_base, bits, nearest=False):
    """buf [C, n] and master [n]: CPU tensors in their storage dtype.
    Returns fp64 arrays [C, n]: d, a (the element's bucket maximum), t,
    u, lvl (the reference's level), Q, and amb (bool).  nearest: the
    round-to-nearest mutant, l = floor(t + 1/2)."""
    L = levels(bits)
    C, n = buf.shape
    d = (buf.float() - master.float().unsqueeze(0)).double().numpy()
    pad = (-n) % BUCKET
    ab = np.abs(np.pad(d, ((0, 0), (0, pad)))).reshape(C, -1, BUCKET)
    a = np.repeat(ab.max(axis=2), BUCKET, axis=1)[:, :n]
    safe = np.where(a == 0, 1.0, a)
    t = np.abs(d) * L / safe
    u = uniform(key, cids, np.uint64(elem_base) + np.arange(n, dtype=np.uint64))
    fl = np.floor(t)
    frac = t - fl
    if nearest:
        lvl = np.minimum(L, np.floor(t + 0.5))
    else:
        lvl = np.minimum(L, fl + (u < frac))
    Q = np.sign(d) * lvl * (a / L)
    amb = (np.abs(frac - u) < AMBIGUOUS) & (a > 0)
    return {"d": d, "a": a, "t": t, "u": u, "lvl": lvl, "Q": Q, "amb": amb,
            "L": L}


def make_case(n, dtype, near, seed, C=1, offset=0):
    """(buf [C, n], master [n]) on the CPU, drawn on the CPU so that a
    seed's properties can be checked without a GPU.  near: the engine's
    regime, replicas within 1e-3 of the master.  From n = 1024 the second
    bucket of every client equals the master.  offset: master is a view
    that many elements into a larger tensor."""
    g = torch.Generator().manual_seed(seed)
    big = torch.randn(n + offset, generator=g).to(dtype)
    master = big[offset:]
    noise = torch.randn(C, n, generator=g)
    buf = (master.float() + 1e-3 * noise if near else noise).to(dtype)
    if n >= 2 * BUCKET:
        buf[:, BUCKET:2 * BUCKET] = master[BUCKET:2 * BUCKET]
    return buf.contiguous(), master


def ambiguous_cap(n):
    return max(1, n // 1000)


def check_choice(got, ref, label=""):
    """got: fp64 [n], what delta holds after one client of weight 1 was
    accumulated into zeros, i.e. Q itself; ref: quantise() of that client
    (C = 1).  Returns the number of ambiguous elements."""
    got = np.asarray(got, dtype=np.float64).reshape(-1)
    d, a, t, L = ref["d"][0], ref["a"][0], ref["t"][0], ref["L"]
    amb = ref["amb"][0]
    n = got.size
    n_amb = int(amb.sum())
    print(f"choice[{label}] n={n} ambiguous={n_amb} "
          f"(cap {ambiguous_cap(n)})")
    assert n_amb <= ambiguous_cap(n), (label, n_amb)
    assert np.isfinite(got).all(), label
    zero = a == 0
    assert (got[zero] == 0).all(), f"{label}: a == 0 bucket is not zero"
    live = ~zero
    x = got[live] * L / a[live]
    lv = np.rint(x)
    assert (np.abs(x - lv) <= 2.0 ** -20 * np.maximum(1.0, np.abs(lv))).all(), \
        f"{label}: got * L / a is not an integer"
    assert (np.abs(lv) <= L).all(), f"{label}: level beyond L"
    dl = d[live]
    assert (np.sign(lv)[lv != 0] == np.sign(dl)[lv != 0]).all(), \
        f"{label}: sign does not follow d"
    assert (lv[dl == 0] == 0).all(), f"{label}: d == 0 left zero"
    tl = t[live]
    fl = np.floor(tl)
    mag = np.abs(lv)
    assert ((mag == fl) | (mag == np.minimum(L, fl + 1))).all(), \
        f"{label}: level is no neighbour of t"
    clear = ~amb[live]
    bad = int((mag[clear] != ref["lvl"][0][live][clear]).sum())
    assert bad == 0, f"{label}: {bad} unexplained choices"
    top = np.abs(dl) == a[live]
    ulp = np.spacing(a[live][top].astype(np.float32)).astype(np.float64)
    assert (np.abs(np.abs(got[live][top]) - a[live][top]) <= 2 * ulp).all(), \
        f"{label}: the bucket's maximum does not return +-a"
    return n_amb
