"""HIP kernels of per-client update clipping (ops/csrc/clip.hip), the
accumulate with its weight sum on the device, and the clipped engine on
the GPU.  Every kernel result is compared with fp64 computed from upcast
copies of the tensors the kernel received, under kernel_bounds.bound."""

import pytest
import torch

import kernel_bounds as kb

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
# 51200 splits into several tiles on the vector path at every C below;
# 100003 does on the scalar path and 100008 on the vector path, both with
# a partial last tile
SQ_N = [1, 7, 450, 1728, 51200, 100003, 100008]


@pytest.fixture(scope="module")
def ops():
    from olearning_sim_amd.ops import load_hip_ops
    return load_hip_ops(required=True)


def _sq_inputs(C, n, dtype, near, seed, offset=0):
    """(buf [C*n], master [n], sq0 [C]) on the GPU.  near: the engine's
    regime, replicas within 1e-3 of the master.  offset: master is a view
    that many elements into a larger tensor."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    big = torch.randn(n + offset, generator=g, device="cuda").to(dtype)
    master = big[offset:]
    noise = torch.randn(C, n, generator=g, device="cuda")
    buf = (master.float() + 1e-3 * noise if near else noise).to(dtype)
    sq0 = torch.rand(C, generator=g, device="cuda") + 0.5
    return buf.reshape(-1).contiguous(), master, sq0


def _sq_ref(buf, master, sq0, C):
    d = kb.upcast(buf).view(C, -1) - kb.upcast(master).unsqueeze(0)
    return kb.upcast(sq0) + (d * d).sum(dim=1)


def _vec(buf, master, n):
    v = 16 // buf.element_size()
    ok = n % v == 0 and buf.data_ptr() % 16 == 0 and master.data_ptr() % 16 == 0
    return v if ok else 1


@pytest.mark.parametrize("near", [False, True], ids=["random", "near"])
@pytest.mark.parametrize("C", [1, 5, 70])
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_sqnorm_bounded_and_deterministic(ops, dtype, C, near):
    for n in SQ_N:
        buf, master, sq0 = _sq_inputs(C, n, dtype, near, seed=n + C)
        sq, again = sq0.clone(), sq0.clone()
        ops.client_delta_sqnorm(sq, buf, master, C)
        ops.client_delta_sqnorm(again, buf, master, C)
        ref = _sq_ref(buf, master, sq0, C)
        # every term is non-negative: scale = ref; the subtraction and the
        # square round once each on top of the n-term sum and the +=
        kb.assert_bounded(sq, ref, ref, n + 4, torch.float32,
                          label=f"sqnorm.{dtype}.C{C}.n{n}")
        assert torch.equal(sq, again), f"n={n}: two calls differ"
        if near:
            # the hoisted form would have cancelled: the sum is far below
            # the |buf|^2 it would have been taken from
            assert float((sq - sq0).max()) < 1e-2 * max(n, 100)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_sqnorm_splits_rows_over_tiles(ops, dtype):
    """The sizes above that are meant to reach the two-kernel form do."""
    v = 16 // torch.empty(0, dtype=dtype).element_size()
    for C in (1, 5, 70):
        assert ops.sqnorm_tiles(51200, C, v) > 1
        assert ops.sqnorm_tiles(100008, C, v) > 1 and 100008 % (256 * v)
        assert ops.sqnorm_tiles(100003, C, 1) > 1 and 100003 % 256
    assert ops.sqnorm_tiles(1728, 70, v) == 1
    # a tiny row at many clients stays one block per client
    assert ops.sqnorm_tiles(64, 1250, v) == 1
    # a 23 M-element row at 125 clients fills the chip
    assert 125 * ops.sqnorm_tiles(23_000_000, 125, v) >= 2048


@pytest.mark.parametrize("dtype,offset", [(torch.bfloat16, 3),
                                          (torch.float16, 5),
                                          (torch.float32, 1)], ids=str)
def test_sqnorm_master_view_at_odd_offset(ops, dtype, offset):
    """master as the engine passes it: a view into the flat cast at an
    element offset that is no multiple of 16 bytes.  n itself would allow
    the vector path."""
    C, n = 5, 51200
    buf, master, sq0 = _sq_inputs(C, n, dtype, True, seed=9, offset=offset)
    assert master.data_ptr() % 16 != 0 and _vec(buf, master, n) == 1
    sq = sq0.clone()
    ops.client_delta_sqnorm(sq, buf, master, C)
    ref = _sq_ref(buf, master, sq0, C)
    kb.assert_bounded(sq, ref, ref, n + 4, torch.float32,
                      label=f"sqnorm.view.{dtype}")


def test_sqnorm_list_form_sums_over_parameters():
    from olearning_sim_amd.ops import fused
    from test_ops_gpu import SHAPES
    C = 5
    g = torch.Generator(device="cuda").manual_seed(4)
    glob = [torch.randn(*s, generator=g, device="cuda").to(torch.bfloat16)
            for s in SHAPES]
    cli = [(m.float().unsqueeze(0) + 1e-2 * torch.randn(
        C, *m.shape, generator=g, device="cuda")).to(torch.bfloat16)
        for m in glob]
    sq = fused.client_delta_sqnorm(cli, glob)
    ref = sum(((kb.upcast(c) - kb.upcast(m).unsqueeze(0)) ** 2)
              .reshape(C, -1).sum(1) for c, m in zip(cli, glob))
    P = sum(m.numel() for m in glob)
    kb.assert_bounded(sq, ref, ref, P + 4 * len(glob), torch.float32,
                      label="sqnorm.list")


def test_sqnorm_rejects_bad_operands(ops):
    sq = torch.zeros(4, device="cuda")
    buf = torch.zeros(4 * 8, device="cuda", dtype=torch.bfloat16)
    master = torch.zeros(8, device="cuda", dtype=torch.bfloat16)
    ops.client_delta_sqnorm(sq, buf, master, 4)
    for bad in [(sq, buf, master.float(), 4), (sq, buf[:-8], master, 4),
                (sq[:3], buf, master, 4), (sq.double(), buf, master, 4)]:
        with pytest.raises(RuntimeError, match="client_delta_sqnorm"):
            ops.client_delta_sqnorm(*bad)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# clip_weights

S_CLIP = 1.5                    # S*S = 2.25 is exact in fp32


def _clip_inputs(C, seed=0):
    """sq below, exactly at, one ulp above and far above S^2, one 0; unit,
    zero and fractional weights."""
    g = torch.Generator().manual_seed(seed)
    sq = torch.rand(C, generator=g) * 6.0
    w = torch.rand(C, generator=g)
    fixed_sq = [9.0, 0.0, 2.25, 2.2500002, 1.0, 1e6, 2.2499998]
    fixed_w = [1.0, 1.0, 0.5, 1.0, 0.0, 0.37, 1.0]
    k = min(C, len(fixed_sq))
    sq[:k] = torch.tensor(fixed_sq[:k])
    w[:k] = torch.tensor(fixed_w[:k])
    w[k::5] = 0.0
    w[k + 1::5] = 1.0
    return sq.cuda(), w.cuda()


@pytest.mark.parametrize("C", [1, 70, 5000])
def test_clip_weights_bounded(ops, C):
    sq, w = _clip_inputs(C)
    w_eff, wsum = ops.clip_weights(sq, w, S_CLIP)
    assert w_eff.shape == (C,) and wsum.shape == (1,)
    assert w_eff.dtype == wsum.dtype == torch.float32
    q = kb.upcast(sq)
    s = torch.where(q > S_CLIP * S_CLIP, S_CLIP / q.sqrt(),
                    torch.ones_like(q))
    ref = kb.upcast(w) * s
    kb.assert_bounded(w_eff, ref, ref.abs(), 1, torch.float32,
                      intrinsic=True, label=f"clip.w_eff.C{C}")
    below = (q <= S_CLIP * S_CLIP).cuda()
    assert torch.equal(w_eff[below], w[below])      # s_c is exactly 1
    if C >= 70:
        assert int(below.sum()) >= 3 and int((~below).sum()) >= 3
        assert float(w_eff[1]) == 1.0               # sq == 0
    we = kb.upcast(w_eff)
    assert abs(float(kb.upcast(wsum)) - float(we.sum())) \
        <= (C + 2) * 2.0 ** -23 * float(we.abs().sum())
    w2, s2 = ops.clip_weights(sq, w, S_CLIP)
    assert torch.equal(w2, w_eff) and torch.equal(s2, wsum)


def test_clip_weights_huge_bound_is_identity(ops):
    """S = 1e30: S*S overflows to inf in fp32 and nothing is above it."""
    sq, w = _clip_inputs(70)
    w_eff, wsum = ops.clip_weights(sq, w, 1e30)
    assert torch.equal(w_eff, w)


# ---------------------------------------------------------------------------
# accumulate with the weight sum on the device

def _accum_case(shapes, C, dtype, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    glob = [torch.randn(*s, generator=g, device="cuda").to(dtype)
            for s in shapes]
    cli = [(m.float().unsqueeze(0) + 0.1 * torch.randn(
        C, *m.shape, generator=g, device="cuda")).to(dtype) for m in glob]
    delta = [torch.randn(*s, generator=g, device="cuda") for s in shapes]
    w = torch.rand(C, generator=g, device="cuda")
    w[::3] = 0.0
    sq = torch.rand(C, generator=g, device="cuda") * 6.0
    return glob, cli, delta, w, sq


def _check_delta(got, delta0, buf, master, w_eff, C, label):
    n = master.numel()
    ref, _, scale_h = kb.delta_math(
        kb.upcast(delta0).reshape(-1), kb.upcast(buf).reshape(-1),
        kb.upcast(master).reshape(-1), kb.upcast(w_eff), [0, n], C,
        hoisted=True)
    kb.assert_bounded(got.reshape(-1), ref, scale_h, C, torch.float32,
                      label=label)


@pytest.mark.parametrize("C", [7, 70])
@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_accum_device_wsum_every_route(ops, dtype, C):
    """List form, one launch per parameter.  bf16 at C = 70 takes the two
    client-parallel kernels (n % 8 == 0 and not); bf16 and fp16 at C = 7
    the vector kernel, with the 7-element bias on the block-table kernel;
    fp32 the block-table kernel throughout."""
    from olearning_sim_amd.ops import fused
    from test_ops_gpu import SHAPES
    shapes = list(SHAPES) + [(450,)]
    glob, cli, delta, w, sq = _accum_case(shapes, C, dtype, seed=C)
    w_eff, wsum = ops.clip_weights(sq, w, S_CLIP)
    delta0 = [d.clone() for d in delta]
    fused.weighted_delta_accum(delta, cli, glob, w_eff, wsum=wsum)
    for i, s in enumerate(shapes):
        _check_delta(delta[i], delta0[i], cli[i], glob[i], w_eff, C,
                     f"accum_dw.{dtype}.C{C}.{s}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=str)
def test_accum_device_wsum_flat_multi_block(ops, dtype):
    """The engine's flat layout: several parameter blocks in one launch."""
    from olearning_sim_amd.ops import fused
    from test_ops_gpu import SHAPES, _layout
    C = 7
    buf, _, master, offs = _layout(SHAPES, C, dtype)
    g = torch.Generator(device="cuda").manual_seed(2)
    w = torch.rand(C, generator=g, device="cuda")
    sq = torch.rand(C, generator=g, device="cuda") * 6.0
    w_eff, wsum = ops.clip_weights(sq, w, S_CLIP)
    delta = torch.randn(master.numel(), generator=g, device="cuda")
    delta0 = delta.clone()
    fused.weighted_delta_accum_flat(delta, buf, master, w_eff, C,
                                    offsets=offs, wsum=wsum)
    ref, _, scale_h = kb.delta_math(
        kb.upcast(delta0), kb.upcast(buf), kb.upcast(master),
        kb.upcast(w_eff), offs.tolist(), C, hoisted=True)
    kb.assert_bounded(delta, ref, scale_h, C, torch.float32,
                      label=f"accum_dw.flat.{dtype}")


def test_accum_device_wsum_matches_host_wsum(ops):
    """Same weights, same sum, same kernel: bit-identical below 64 clients
    (from 64 the client-parallel kernels add with float atomics)."""
    from olearning_sim_amd.ops import fused
    C, n = 8, 4096
    glob, cli, delta, w, _ = _accum_case([(n,)], C, torch.bfloat16, seed=3)
    wsum = w.sum().reshape(1)
    d_host, d_dev = delta[0].clone(), delta[0].clone()
    fused.weighted_delta_accum([d_host], cli, glob, w, wsum=float(wsum))
    fused.weighted_delta_accum([d_dev], cli, glob, w, wsum=wsum)
    assert torch.equal(d_host, d_dev)


def test_accum_device_wsum_rejects_host_tensor(ops):
    n, C = 8, 2
    args = (torch.zeros(n, device="cuda"),
            torch.zeros(C * n, device="cuda"), torch.zeros(n, device="cuda"),
            torch.ones(C, device="cuda"),
            torch.tensor([0, n], device="cuda"), C)
    with pytest.raises(RuntimeError, match="wsum"):
        ops.weighted_delta_accum_flat_dw(*args, torch.ones(1))
    with pytest.raises(RuntimeError, match="wsum"):
        ops.weighted_delta_accum_flat_dw(*args, torch.ones(2, device="cuda"))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# engine: bf16 MLP, 8 clients (below 64, so every accumulate is
# run-to-run identical)

def _engine(**kw):
    from olearning_sim_amd.engine import EngineJob, LogicalEngine
    base = dict(task_id="t_clip_gpu", model_name="mlp",
                model_kwargs={"in_features": 64, "hidden": 32,
                              "num_classes": 10},
                clients=8, rounds=2, local_steps=2, batch_size=8, lr=0.1,
                device="cuda:0", dtype="bfloat16", num_classes=10, seed=5)
    base.update(kw)
    return LogicalEngine(EngineJob(**base))


def test_engine_huge_clip_norm_is_bit_identical_to_off():
    """clip_norm = 1e30: every s_c is exactly 1 and the sums of 0/1
    weights are exact, so the whole clipped path must reproduce the plain
    one bit for bit."""
    plain, huge = _engine(), _engine(clip_norm=1e30)
    for r in range(2):
        plain.run_round(r)
        rec = huge.run_round(r)
        assert rec["clipped"] == 0 and rec["update_norm_mean"] > 0
    assert torch.equal(plain.master.flat, huge.master.flat)


def test_engine_clipped_update_is_norm_bounded():
    """With S a quarter of the unclipped round's master step, the clipped
    step must come out no longer than S.

    In exact arithmetic delta_master = (1/W) sum_c w_c s_c delta_c with
    w_c = 1, W = C, and ||s_c delta_c|| <= S, so ||delta_master|| <= S.

    Relative term (P + C + 8) 2^-23: s_c = S / sqrtf(sq_c), and sq_c is an
    fp32 sum of P squared differences, off by at most (P + 4) 2^-23
    relative, which the square root halves; the square root, the divide,
    the product w_c s_c and the final delta / W round once each (4 2^-24);
    the C-term sum of the scaled updates adds (C + 2) 2^-23.  Together
    below (P + C + 8) 2^-23.

    Absolute term E = (C + 2) 2^-22 (||master|| + S): the kernel does not
    sum s_c delta_c, it evaluates sum_c w_eff_c buf_c - wsum_eff master in
    fp32.  Each of the two sums carries (C + 2) 2^-23 of its abs-value
    scale, per coordinate W (|master_j| + |s_c delta_cj|) at most; after
    the division by W and in the 2-norm that is (C + 2) 2^-23
    (||master|| + S) each, 2^-22 for both."""
    plain = _engine(rounds=1)
    m0 = plain.master.flat.double().clone()
    plain.run_round(0)
    step = float((plain.master.flat.double() - m0).norm())
    S = step / 4

    clipped = _engine(rounds=1, clip_norm=S)
    assert torch.equal(clipped.master.flat.double(), m0)
    rec = clipped.run_round(0)
    got = float((clipped.master.flat.double() - m0).norm())
    P, C = m0.numel(), 8
    E = (C + 2) * 2.0 ** -22 * (float(m0.norm()) + S)
    limit = S * (1 + (P + C + 8) * 2.0 ** -23) + E
    print(f"unclipped step {step:.6g}, S {S:.6g}, clipped step {got:.6g}, "
          f"limit {limit:.6g}")
    assert 0 < got <= limit
    assert rec["clipped"] == 8
    assert rec["update_norm_mean"] > S


def test_engine_noise_on_gpu_is_reproducible():
    a = _engine(rounds=1, clip_norm=0.05, noise_multiplier=1.0)
    b = _engine(rounds=1, clip_norm=0.05, noise_multiplier=1.0)
    c = _engine(rounds=1, clip_norm=0.05)
    for e in (a, b, c):
        e.run_round(0)
    assert torch.equal(a.master.flat, b.master.flat)
    noise = (a.master.flat - c.master.flat).double()
    sigma = 1.0 * 0.05 / 8
    # sampling error of a standard deviation over P draws, plus the fp32
    # rounding of master + noise (2^-24 |master|, far below sigma)
    assert abs(float(noise.std()) - sigma) \
        <= 5 / (2 * noise.numel()) ** 0.5 * sigma
