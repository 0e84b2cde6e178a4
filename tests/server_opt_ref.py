"""Reference math, inputs and bounds of the server optimiser step, shared
by test_server_opt_cpu.py and test_server_opt_gpu.py.

The rule (ops/fused.py server_opt_step), with g = d*(1/W) + sigma*z:

    momentum: m = b1*m + g;            x += lr*m
    adagrad:  m = b1*m + (1-b1)*g;     v = v + g^2
    adam:     same m;                  v = b2*v + (1-b2)*g^2
    yogi:     same m;                  v = v - (1-b2)*g^2*sign(v - g^2)
    adaptive: x += lr*m / (sqrt(v) + tau)

``step_math`` evaluates it in the dtype of its tensors: in fp64 on
``kernel_bounds.upcast`` copies as the reference, in fp32 as a stand-in
kernel whose mutants the bounds must reject.  The scalars are the fp32
values the kernel receives, upcast.

Bounds (kernel_bounds.assert_bounded), with sg = |d|/W + sigma|z| the
scale of g:

- m: scale b1|m0| + c*sg (c = 1 for momentum, 1-b1 otherwise), n = 6
- v: scale |v0| + sg^2, n = 8.  No kind cancels here: Yogi's result is at
  least b2*v0 where v0 > g^2.
- x: scale |x0| + lr*scale_m/(sqrt(v)+tau) (denominator 1 for momentum),
  n = 16

Yogi is discontinuous where v0 = g^2.  The fp32 g carries up to three
roundings of sg (the product d*(1/W), sigma*z, their sum), its square so
up to 6*2^-24 sg^2 and one more for the square itself, and the difference
v0 - g^2 one rounding of |v0| + sg^2: below 2^-21 (sg^2 + |v0|) in all.
Elements whose fp64 |v0 - g^2| is not above that are undecided and left
out of the v and x checks; ``yogi_decided`` asserts they are at most 1 in
1000 and, from 100 elements on, that each sign holds at least 10 % of the
rest (with 1 to 7 elements a share of 10 % means nothing).
"""

from __future__ import annotations

import torch

import kernel_bounds as kb

KINDS = ("momentum", "adagrad", "adam", "yogi")
SIZES = (1, 3, 4, 7, 450, 1028, 100003, 100008)

W = 3.0
SIGMA = 0.01
LR = 0.1
B1 = 0.9
B2 = 0.99
TAU = 1e-3


def f32(v) -> float:
    """The value a launcher receives when handed the Python float v."""
    return float(torch.tensor(float(v), dtype=torch.float32))


def scalars(total_weight=W, sigma=SIGMA, lr=LR, b1=B1, b2=B2, tau=TAU):
    """The step's scalars at their fp32 values."""
    return {"inv_w": f32(1.0 / total_weight), "sigma": f32(sigma),
            "lr": f32(lr), "b1": f32(b1), "b2": f32(b2), "tau": f32(tau)}


_INPUTS: dict = {}


def inputs(n, seed=0):
    """CPU fp32 (x, d, m, v, z) of n elements, built once per (n, seed)
    and never written to: Gaussian x, d (std 3), m (std 0.3), v in
    [0.25, 2.25] with every 100th element at 1e-6 (tau decides the
    denominator there), standard normal z."""
    key = (n, seed)
    if key not in _INPUTS:
        g = torch.Generator().manual_seed(1000 * seed + n)
        x = torch.randn(n, generator=g)
        d = 3.0 * torch.randn(n, generator=g)
        m = 0.3 * torch.randn(n, generator=g)
        v = 0.25 + 2.0 * torch.rand(n, generator=g)
        v[::100] = 1e-6
        z = torch.randn(n, generator=g)
        _INPUTS[key] = (x, d, m, v, z)
    return _INPUTS[key]


def step_math(kind, x, d, m, v, z, sc, mutant=None):
    """One step in the dtype of the tensors.  z None: no noise.  Returns
    the new x, m, v (v None for momentum), g, and the three scales.
    Mutants: "no_tau" drops tau from the denominator, "flip_sign" flips
    Yogi's sign."""
    g = d * sc["inv_w"]
    sg = d.abs() * sc["inv_w"]
    if z is not None:
        g = g + sc["sigma"] * z
        sg = sg + sc["sigma"] * z.abs()
    b1, b2, lr, tau = sc["b1"], sc["b2"], sc["lr"], sc["tau"]
    if kind == "momentum":
        m1 = b1 * m + g
        m_scale = b1 * m.abs() + sg
        return {"x": x + lr * m1, "m": m1, "v": None, "g": g, "sg": sg,
                "m_scale": m_scale, "v_scale": None,
                "x_scale": x.abs() + lr * m_scale}
    m1 = b1 * m + (1 - b1) * g
    m_scale = b1 * m.abs() + (1 - b1) * sg
    g2 = g * g
    if kind == "adagrad":
        v1 = v + g2
    elif kind == "adam":
        v1 = b2 * v + (1 - b2) * g2
    else:
        sign = torch.sign(v - g2)
        if mutant == "flip_sign":
            sign = -sign
        v1 = v - (1 - b2) * g2 * sign
    den = v1.sqrt() if mutant == "no_tau" else v1.sqrt() + tau
    return {"x": x + lr * m1 / den, "m": m1, "v": v1, "g": g, "sg": sg,
            "m_scale": m_scale, "v_scale": v.abs() + sg * sg,
            "x_scale": x.abs() + lr * m_scale / (v1.sqrt() + tau)}


def reference(kind, x, d, m, v, z, sc):
    """step_math in fp64 on upcast copies of the tensors passed."""
    up = [None if t is None else kb.upcast(t) for t in (x, d, m, v, z)]
    if kind == "momentum":
        up[3] = None
    return step_math(kind, *up, sc)


def yogi_decided(ref, v0, label="", shares=True):
    """Mask of the elements whose Yogi sign fp64 decides (module
    docstring), with its two conditions asserted.  shares=False drops the
    second one, for inputs a test does not choose (an engine's delta)."""
    g2 = ref["g"] * ref["g"]
    diff = kb.upcast(v0) - g2
    tol = 2.0 ** -21 * (ref["sg"] * ref["sg"] + kb.upcast(v0).abs())
    dec = diff.abs() > tol
    n = dec.numel()
    excluded = n - int(dec.sum())
    pos = int((dec & (diff > 0)).sum())
    neg = int((dec & (diff < 0)).sum())
    print(f"yogi[{label}] excluded {excluded} of {n}, v0 > g^2 in "
          f"{pos}, v0 < g^2 in {neg}")
    assert excluded <= n / 1000, f"{label}: {excluded} of {n} undecided"
    if shares and n >= 100:
        rest = n - excluded
        assert pos >= 0.1 * rest and neg >= 0.1 * rest, (label, pos, neg)
    return dec


def assert_step_bounded(kind, got_x, got_m, got_v, ref, v0, label,
                        shares=True):
    """got_*: the tensors after the step; ref: reference() of the tensors
    before it.  Returns the worst err/bound per tensor."""
    where = (yogi_decided(ref, v0, label, shares) if kind == "yogi"
             else None)
    worst = {"m": kb.assert_bounded(got_m, ref["m"], ref["m_scale"], 6,
                                    torch.float32, label=label + ".m")}
    if kind != "momentum":
        worst["v"] = kb.assert_bounded(got_v, ref["v"], ref["v_scale"], 8,
                                       torch.float32, where=where,
                                       label=label + ".v")
    worst["x"] = kb.assert_bounded(got_x, ref["x"], ref["x_scale"], 16,
                                   torch.float32, where=where,
                                   label=label + ".x")
    return worst
