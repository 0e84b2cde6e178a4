"""HIP kernels of the quantised accumulate (ops/csrc/uplink_quant.hip)
and the engine with uplink compression on the GPU.  The reference is the
independent fp64 implementation of the contract in uplink_ref.py, run on
upcast copies of the tensors the kernel received; sums are held to
kernel_bounds.bound."""

import numpy as np
import pytest
import torch

import kernel_bounds as kb
import uplink_ref as ur

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
# 100003 takes the scalar route, 100008 the vector route with a partial
# last bucket
CHOICE_N = [1, 7, 450, 512, 513, 1728, 100003, 100008]
CIDS = [0, 5, 2 ** 31 + 3]
KEY = (0x0BADF00D << 32) | 0x1234ABCD
K0, K1 = KEY & ur.M32, KEY >> 32


@pytest.fixture(scope="module")
def ops():
    from olearning_sim_amd.ops import load_hip_ops
    return load_hip_ops(required=True)


def _dt(dtype):
    return DTYPES.index(dtype)


def _route(ops, buf, master, C):
    return ops.delta_accum_quant_route(
        master.numel(), C, _dt(master.dtype), master.data_ptr() % 16 == 0,
        buf.data_ptr() % 16 == 0)


def _run(ops, buf, master, w, cids, bits, base, delta0=None, key=KEY):
    """One launch on GPU copies of CPU operands; master keeps its view
    offset.  Returns (delta on the GPU, route name)."""
    C, n = buf.shape
    gbuf = buf.cuda().reshape(-1)
    off = master.storage_offset()
    gmaster = master._base.cuda()[off:] if master._base is not None \
        else master.cuda()
    delta = torch.zeros(n, device="cuda") if delta0 is None \
        else delta0.cuda().clone()
    ops.delta_accum_quant(delta, gbuf, gmaster,
                          torch.as_tensor(w, dtype=torch.float32).cuda(),
                          torch.as_tensor(cids, dtype=torch.int64).cuda(), C,
                          bits, key & ur.M32, key >> 32, base)
    return delta, _route(ops, gbuf, gmaster, C)


# ---------------------------------------------------------------------------
# 1. per-element choice

def _choice_cases():
    """(n, near, cid, elem_base): every small n with every combination;
    the two large ones with every regime, id and base, not crossed."""
    out = []
    for n in CHOICE_N:
        if n < 10000:
            out += [(n, near, cid, base) for near in (False, True)
                    for cid in CIDS for base in (0, ur.BIG_BASE)]
        else:
            out += [(n, near, cid, base) for near in (False, True)
                    for cid, base in zip(CIDS, (0, ur.BIG_BASE, ur.BIG_BASE))]
    return out


@pytest.mark.parametrize("bits", [2, 4, 8])
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_kernel_makes_the_contracts_choice(ops, dtype, bits):
    """C = 1, w = [1], delta0 = 0: the output is Q itself.  The seeds are
    those of the CPU test, where the reference alone is shown to stay
    under the cap of the ambiguous set."""
    routes = set()
    for n, near, cid, base in _choice_cases():
        buf, master = ur.make_case(n, dtype, near, seed=n + 3 * near)
        ref = ur.quantise(buf, master, KEY, [cid], base, bits)
        delta, route = _run(ops, buf, master, [1.0], [cid], bits, base)
        routes.add((n % 8 == 0, route))
        ur.check_choice(
            kb.upcast(delta).numpy(), ref,
            f"{dtype}.b{bits}.n{n}.near{int(near)}.cid{cid}.base{base}")
        if n >= 2 * ur.BUCKET:
            # the bucket where buf == master
            assert not delta[ur.BUCKET:2 * ur.BUCKET].any()
    assert routes == {(True, "v8"), (False, "scalar")}


def test_equal_rows_add_exact_zeros(ops):
    for n in (7, 512, 1032):
        _, master = ur.make_case(n, torch.bfloat16, False, seed=n)
        buf = master.unsqueeze(0).expand(3, n).contiguous()
        delta, _ = _run(ops, buf, master, [1.0, 2.0, 0.5], [1, 2, 3], 4, 0)
        assert not delta.any()


# ---------------------------------------------------------------------------
# 2. accumulate

ACC_N = [7, 450, 1728, 4099, 4104]      # 4104 = 8 * 513: a partial bucket


def _accum_ref(buf, master, w, cids, bits, base, delta0, key=KEY):
    C = buf.shape[0]
    ref = ur.quantise(buf, master, key, np.asarray(cids), base, bits)
    w64 = torch.as_tensor(w, dtype=torch.float32).double().numpy() \
        .reshape(C, 1)
    d0 = delta0.double().numpy()
    want = d0 + (w64 * ref["Q"]).sum(axis=0)
    scale = np.abs(d0) + (np.abs(w64) * np.abs(ref["Q"])).sum(axis=0)
    amb = ref["amb"] & (w64 != 0)
    # one level of every ambiguous client
    extra = (np.abs(w64) * amb * ref["a"] / ref["L"]).sum(axis=0)
    return (torch.from_numpy(want), torch.from_numpy(scale),
            torch.from_numpy(~amb.any(axis=0)), torch.from_numpy(extra))


@pytest.mark.parametrize("bits", [2, 4, 8])
@pytest.mark.parametrize("C", [7, 70])
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_accumulate_bounded(ops, dtype, C, bits):
    """Weights with zeros, a random delta0.  C = 70 takes two client tiles
    and float atomics."""
    g = torch.Generator().manual_seed(C + bits)
    w = torch.rand(C, generator=g)
    w[::3] = 0.0
    cids = (torch.arange(C, dtype=torch.int64) * 3 + 1).tolist()
    excluded = total = 0
    for n in ACC_N:
        buf, master = ur.make_case(n, dtype, True, seed=n + C, C=C)
        delta0 = torch.randn(n, generator=g)
        want, scale, clear, extra = _accum_ref(buf, master, w, cids, bits,
                                               6, delta0)
        excluded += int((~clear).sum())
        total += n
        delta, _ = _run(ops, buf, master, w, cids, bits, 6, delta0)
        label = f"quant_accum.{dtype}.C{C}.b{bits}.n{n}"
        kb.assert_bounded(delta, want, scale, C, torch.float32, where=clear,
                          label=label)
        kb.assert_bounded(delta, want, scale, C, torch.float32, extra=extra,
                          label=label + ".all")
    share = excluded / total
    print(f"coordinates with an ambiguous client: {share:.2e}")
    assert share <= (0.005 if C == 7 else 0.03)


# ---------------------------------------------------------------------------
# 3. routes

def test_route_names(ops):
    for dt in range(3):
        for C in (1, 7, 70, 1250):
            assert ops.delta_accum_quant_route(4096, C, dt, True, True) == "v8"
            assert ops.delta_accum_quant_route(4104, C, dt, True, True) == "v8"
            assert ops.delta_accum_quant_route(8, C, dt, True, True) == "v8"
            for n in (1, 7, 450, 4099, 100003):
                assert ops.delta_accum_quant_route(n, C, dt, True, True) \
                    == "scalar"
            assert ops.delta_accum_quant_route(4096, C, dt, False, True) \
                == "scalar"
            assert ops.delta_accum_quant_route(4096, C, dt, True, False) \
                == "scalar"


@pytest.mark.parametrize("dtype,offset", [(torch.bfloat16, 3),
                                          (torch.float16, 5),
                                          (torch.float32, 1)], ids=str)
@pytest.mark.parametrize("C", [7, 70])
def test_master_view_at_odd_offset_takes_the_scalar_route(ops, dtype, offset,
                                                          C):
    """master as the engine passes it: a view into the flat cast at an
    element offset that is no multiple of 16 bytes.  Same data on both
    routes, same draws: both hold to the reference and to each other."""
    n, bits, base = 4104, 4, 2 * 4104
    buf, master = ur.make_case(n, dtype, True, seed=11, C=C, offset=offset)
    aligned = master.clone()
    g = torch.Generator().manual_seed(offset)
    w = torch.rand(C, generator=g)
    cids = list(range(40, 40 + C))
    delta0 = torch.randn(n, generator=g)
    want, scale, clear, extra = _accum_ref(buf, master, w, cids, bits, base,
                                           delta0)
    d_s, r_s = _run(ops, buf, master, w, cids, bits, base, delta0)
    d_v, r_v = _run(ops, buf, aligned, w, cids, bits, base, delta0)
    assert (r_s, r_v) == ("scalar", "v8")
    for got, name in ((d_s, "scalar"), (d_v, "v8")):
        kb.assert_bounded(got, want, scale, C, torch.float32, where=clear,
                          label=f"route.{name}.{dtype}.C{C}")
        kb.assert_bounded(got, want, scale, C, torch.float32, extra=extra,
                          label=f"route.{name}.{dtype}.C{C}.all")
    # against each other: two fp32 sums of the same terms, unless an
    # ambiguous element fell differently
    kb.assert_bounded(d_s, kb.upcast(d_v), scale, 2 * C, torch.float32,
                      extra=extra, roundings=2, label=f"route.pair.{dtype}")


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_odd_elem_base_on_the_vector_route(ops, dtype):
    """An odd base splits a lane's 8 elements over 5 pairs."""
    n, bits, base, C = 1032, 8, 7, 3
    buf, master = ur.make_case(n, dtype, False, seed=5, C=C)
    cids, w = [9, 10, 11], [1.0, 0.5, 2.0]
    delta0 = torch.zeros(n)
    want, scale, clear, extra = _accum_ref(buf, master, w, cids, bits, base,
                                           delta0)
    delta, route = _run(ops, buf, master, w, cids, bits, base)
    assert route == "v8"
    kb.assert_bounded(delta, want, scale, C, torch.float32, where=clear,
                      label=f"oddbase.{dtype}")
    kb.assert_bounded(delta, want, scale, C, torch.float32, extra=extra,
                      label=f"oddbase.{dtype}.all")


# ---------------------------------------------------------------------------
# 4. identity of the draw

def test_draws_follow_ids_and_key_not_the_call(ops):
    n, bits, base = 4104, 4, 4096
    buf, master = ur.make_case(n, torch.bfloat16, True, seed=21, C=8)
    ids = list(range(10, 18))
    w = [1.0, 0.5, 0.25, 2.0, 1.5, 0.75, 1.0, 3.0]
    one, _ = _run(ops, buf, master, w, ids, bits, base)
    again, _ = _run(ops, buf, master, w, ids, bits, base)
    assert torch.equal(one, again)          # C < 64: no atomics
    half, _ = _run(ops, buf[:4], master, w[:4], ids[:4], bits, base)
    two, _ = _run(ops, buf[4:], master, w[4:], ids[4:], bits, base,
                  delta0=half.cpu())
    want, scale, _, _ = _accum_ref(buf, master, w, ids, bits, base,
                                   torch.zeros(n))
    # the same 8 terms summed in two orders
    kb.assert_bounded(two, kb.upcast(one), scale, 2 * 8, torch.float32,
                      roundings=2, label="draw.split")
    other_id, _ = _run(ops, buf, master, w, [99] + ids[1:], bits, base)
    other_key, _ = _run(ops, buf, master, w, ids, bits, base, key=KEY + 1)
    other_k1, _ = _run(ops, buf, master, w, ids, bits, base,
                       key=KEY + (1 << 32))
    other_base, _ = _run(ops, buf, master, w, ids, bits, base + 2)
    for other in (other_id, other_key, other_k1, other_base):
        assert not torch.equal(one, other)


# ---------------------------------------------------------------------------
# 5. unbiasedness

@pytest.mark.parametrize("bits", [2, 8])
def test_mean_over_many_clients_is_the_update(ops, bits):
    """C identical rows under ids 0..C-1, w = 1/C: the output is the mean
    of C independent draws of Q.  A draw has variance at most (a/L)^2 / 4
    (two neighbouring levels a/L apart), so each coordinate's mean lies
    within 6 sigma = 6 (a/L) / (2 sqrt C) of d, plus the fp32 sum."""
    C, n = 4096, 2048
    row, master = ur.make_case(n, torch.bfloat16, False, seed=31)
    L = ur.levels(bits)
    d = (row.float() - master.float().unsqueeze(0)).double()[0]
    a = d.abs().view(-1, ur.BUCKET).max(dim=1).values \
        .repeat_interleave(ur.BUCKET)
    buf = row.expand(C, n).contiguous()
    w = torch.full((C,), 1.0 / C)
    delta, _ = _run(ops, buf, master, w, list(range(C)), bits, 0)
    got = kb.upcast(delta)
    # sum_c |w_c||Q_c| <= a
    tol = 6 * (a / L) / (2 * C ** 0.5) + kb.bound(d, a, C, torch.float32)
    worst = float(((got - d).abs() / tol)[a > 0].max())
    print(f"unbiased[b{bits}] worst |mean - d| / tol = {worst:.3f}")
    assert worst <= 1.0
    if bits == 2:
        # round to nearest, computed here: biased, and the check sees it
        lvl = torch.clamp(torch.floor(d.abs() * L / a + 0.5), max=L)
        mutant = torch.sign(d) * lvl * (a / L)
        assert bool(((mutant - d).abs() > tol)[a > 0].any())
        assert not bool((got == mutant).all())


# ---------------------------------------------------------------------------
# 6. bad operands

def test_bad_operands_raise(ops):
    C, n = 2, 16
    delta = torch.zeros(n, device="cuda")
    buf = torch.zeros(C * n, device="cuda", dtype=torch.bfloat16)
    master = torch.zeros(n, device="cuda", dtype=torch.bfloat16)
    w = torch.ones(C, device="cuda")
    ids = torch.arange(C, device="cuda")
    ops.delta_accum_quant(delta, buf, master, w, ids, C, 4, K0, K1, 0)
    big = torch.tensor([0, 2 ** 32], device="cuda")
    bad = [
        (delta, buf, master.float(), w, ids, C, 4, K0, K1, 0),   # dtypes
        (delta, buf.to(torch.int16), master.to(torch.int16), w, ids, C, 4,
         K0, K1, 0),
        (delta.double(), buf, master, w, ids, C, 4, K0, K1, 0),
        (delta, buf[:-8], master, w, ids, C, 4, K0, K1, 0),      # short buf
        (delta[:-1], buf, master, w, ids, C, 4, K0, K1, 0),
        (delta, buf, master, w[:1], ids, C, 4, K0, K1, 0),
        (delta, buf, master, w, ids.cpu(), C, 4, K0, K1, 0),     # host ids
        (delta, buf, master, w, ids.int(), C, 4, K0, K1, 0),
        (delta, buf, master, w, ids, C, 3, K0, K1, 0),           # bits
        (delta, buf, master, w, ids, C, 0, K0, K1, 0),
        (delta, buf, master, w, big, C, 4, K0, K1, 0),           # cid 2^32
        (delta, buf, master, w, -ids - 1, C, 4, K0, K1, 0),
        (delta, buf, master, w, ids, C, 4, 2 ** 32, K1, 0),
        (delta, buf, master, w, ids, C, 4, K0, K1, 2 ** 33),     # pair index
        (delta, buf, master, w, ids, C, 4, K0, K1, -2),
    ]
    for args in bad:
        with pytest.raises(RuntimeError, match="delta_accum_quant"):
            ops.delta_accum_quant(*args)
    torch.cuda.synchronize()
    assert not delta.any()


# ---------------------------------------------------------------------------
# 7. engine: the bf16 MLP of test_clip_gpu.py, 8 clients (below 64, so
# every accumulate is run-to-run identical)

def _engine(**kw):
    from olearning_sim_amd.engine import EngineJob, LogicalEngine
    base = dict(task_id="t_uplink_gpu", model_name="mlp",
                model_kwargs={"in_features": 64, "hidden": 32,
                              "num_classes": 10},
                clients=8, rounds=2, local_steps=2, batch_size=8, lr=0.1,
                device="cuda:0", dtype="bfloat16", num_classes=10, seed=5)
    base.update(kw)
    return LogicalEngine(EngineJob(**base))


def test_engine_is_reproducible_and_counts_its_bytes():
    plain, a, b = _engine(), _engine(uplink_bits=8), _engine(uplink_bits=8)
    numels = [64 * 32, 32, 32 * 10, 10]
    per = sum(n + 4 * ((n + 511) // 512) for n in numels)
    assert per == ur.bytes_per_client(numels, 8)
    for r in range(2):
        rec0 = plain.run_round(r)
        rec = a.run_round(r)
        b.run_round(r)
        assert not [k for k in rec0 if k.startswith("uplink")]
        assert rec["uplink_bytes_per_client"] == per
        assert rec["uplink_bytes"] == 8 * per
        assert rec["uplink_ratio"] == per / (sum(numels) * 4)
    assert torch.equal(a.master.flat, b.master.flat)
    assert not torch.equal(a.master.flat, plain.master.flat)
    assert bool(torch.isfinite(a.master.flat).all())


def test_engine_huge_clip_norm_changes_nothing():
    """clip_norm = 1e30: every s_c is exactly 1, so the weights the
    quantised accumulate receives are the same bits."""
    alone, huge = _engine(uplink_bits=8), _engine(uplink_bits=8,
                                                  clip_norm=1e30)
    for r in range(2):
        alone.run_round(r)
        assert huge.run_round(r)["clipped"] == 0
    assert torch.equal(alone.master.flat, huge.master.flat)
