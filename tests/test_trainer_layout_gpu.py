"""The trainer's tail under the trainer's operand layout: global
parameters are views into the flat cast at arbitrary element offsets,
delta blocks fp32 views into the flat delta, where every other kernel test
allocates its operands fresh (256-byte aligned).  replicate and the two
vector accumulate kernels load 16 bytes at a time and are unreachable with
a master that does not start on a 16-byte boundary (delta_route.h,
replicate_params); this file asserts each guard, then runs

    cast views -> replicate_params -> 3 x fused_sgd_update ->
    client_delta_sqnorm -> clip_weights -> weighted_delta_accum

on given gradients in bf16, fp16 and fp32, every kernel result against
fp64 from upcast copies of what it received."""

import pytest
import torch

import kernel_bounds as kb

pytestmark = pytest.mark.gpu

BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
CODE = {F32: 0, BF: 1, F16: 2}

# element offsets 0, 3, 67, 72, 1224, 1674, 2514, 133586, 133592: 64 at 3,
# 1152 at 72 (aligned, the control), 840 at 1674 and 131072 at 2514 (both
# 2 mod 8), and behind a 6-element spacer the aligned twin of the 131072
SHAPES = [(3,), (64,), (5,), (16, 8, 3, 3), (450,), (840,), (131072,), (6,),
          (131072,)]
OFFSETS = [0, 3, 67, 72, 1224, 1674, 2514, 133586, 133592]

BT, V8, CPAR, CPAR_S = "block_table", "v8", "cpar", "cpar_s"
# per parameter: (route were the view 16-byte aligned, route it takes).
# 131072 is the first n of a bf16 parameter at >= 64 clients that is not
# client-parallel.  Read off aggregate.hip's launcher by hand.
FEW = [(BT, BT), (V8, BT), (BT, BT), (V8, V8), (BT, BT), (V8, BT), (V8, BT),
       (BT, BT), (V8, V8)]
ROUTES = {
    (BF, 7): FEW, (F16, 7): FEW, (F16, 70): FEW,
    (BF, 70): [(CPAR_S, CPAR_S), (CPAR, CPAR_S), (CPAR_S, CPAR_S),
               (CPAR, CPAR), (CPAR_S, CPAR_S), (CPAR, CPAR_S), (V8, BT),
               (CPAR_S, CPAR_S), (V8, V8)],
    (F32, 7): [(BT, BT)] * 9, (F32, 70): [(BT, BT)] * 9,
}
LR = 0.1


@pytest.fixture(scope="module")
def ops():
    from olearning_sim_amd.ops import load_hip_ops
    return load_hip_ops(required=True)


def _aligned(i, dtype):
    return OFFSETS[i] * torch.empty(0, dtype=dtype).element_size() % 16 == 0


def _numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


def test_route_table_names_every_route_and_both_refusals():
    got = [r for table in ROUTES.values() for r in table]
    assert {taken for _, taken in got} == {BT, V8, CPAR, CPAR_S}
    for vec, scalar in ((V8, BT), (CPAR, CPAR_S)):
        assert (vec, vec) in got, f"{vec} never taken"
        assert (vec, scalar) in got, f"{vec} never refused for alignment"
    # a refusal is an alignment refusal: n % 8 == 0 and the view misaligned
    for (dtype, C), table in ROUTES.items():
        for i, (if_aligned, taken) in enumerate(table):
            if if_aligned != taken:
                assert _numel(SHAPES[i]) % 8 == 0 and not _aligned(i, dtype)
            if dtype != F32 and _numel(SHAPES[i]) % 8 == 0:
                assert (if_aligned == taken) == _aligned(i, dtype)


def test_route_function_on_misaligned_replicas_and_blocks(ops):
    # either operand misaligned refuses the vector kernel
    assert ops.delta_accum_route(1, 1152, 70, 1, True, True) == CPAR
    assert ops.delta_accum_route(1, 1152, 70, 1, True, False) == CPAR_S
    assert ops.delta_accum_route(1, 1152, 70, 1, False, True) == CPAR_S
    assert ops.delta_accum_route(1, 1152, 7, 2, True, False) == BT
    # thresholds of the client-parallel pair: clients 64, n 131072
    assert ops.delta_accum_route(1, 1152, 63, 1, True, True) == V8
    assert ops.delta_accum_route(1, 1152, 64, 1, True, True) == CPAR
    assert ops.delta_accum_route(1, 131064, 64, 1, True, True) == CPAR
    assert ops.delta_accum_route(1, 131071, 64, 1, True, True) == CPAR_S
    assert ops.delta_accum_route(1, 131072, 64, 1, True, True) == V8
    assert ops.delta_accum_route(1, 131073, 64, 1, True, True) == BT
    # several blocks in one launch: the block table, whatever the rest
    assert ops.delta_accum_route(2, 1152, 70, 1, True, True) == BT


def test_replicate_rejects_misaligned_source(ops):
    for dtype, off in ((BF, 3), (BF, 2), (F32, 2), (F32, 1)):
        big = torch.randn(64 + off, device="cuda").to(dtype)
        assert big[off:].data_ptr() % 16 != 0
        with pytest.raises(RuntimeError, match="16-byte"):
            ops.replicate(big[off:], 3)
    # bf16 at 8 elements, fp32 at 4: 16 bytes, accepted
    for dtype, off in ((BF, 8), (F32, 4)):
        big = torch.randn(64 + off, device="cuda").to(dtype)
        rep = ops.replicate(big[off:], 3)
        assert torch.equal(rep, big[off:].unsqueeze(0).expand(3, -1))
    torch.cuda.synchronize()


class _CountReplicate:
    def __init__(self, ops):
        self._ops = ops
        self.sources = []

    def __getattr__(self, name):
        return getattr(self._ops, name)

    def replicate(self, src, clients):
        self.sources.append(src.data_ptr())
        return self._ops.replicate(src, clients)


@pytest.mark.parametrize("mu", [0.0, 0.5])
@pytest.mark.parametrize("C", [7, 70])
@pytest.mark.parametrize("dtype", [BF, F16, F32], ids=str)
def test_trainer_tail_on_flat_views(ops, dtype, C, mu, monkeypatch):
    from olearning_sim_amd.engine.client_manager import (FlatParams,
                                                         replicate_params)
    from olearning_sim_amd.ops import fused
    tag = f"{str(dtype).split('.')[-1]}.C{C}.mu{mu}"
    g = torch.Generator(device="cuda").manual_seed(100 * C + CODE[dtype])
    names = [f"p{i}" for i in range(len(SHAPES))]
    master = FlatParams({k: torch.randn(*s, generator=g, device="cuda")
                         for k, s in zip(names, SHAPES)})
    assert master.offsets.tolist()[:-1] == OFFSETS

    # 1. the cast and its views, as begin_round / _cast_params make them
    cast_flat = master.flat.to(dtype)
    cast = master.views_of(cast_flat)
    glist = [cast[k] for k in names]
    assert cast_flat.data_ptr() % 16 == 0
    for i, gw in enumerate(glist):
        assert (gw.data_ptr() % 16 == 0) == _aligned(i, dtype), names[i]

    # 2. replicas: the broadcast kernel only from a 16-byte aligned view
    proxy = _CountReplicate(ops)
    monkeypatch.setattr(fused, "_HIP_OPS", proxy)
    params = replicate_params(cast, C)
    monkeypatch.setattr(fused, "_HIP_OPS", ops)
    want = [gw.data_ptr() for i, gw in enumerate(glist)
            if dtype != F16 and gw.numel() % 8 == 0 and _aligned(i, dtype)]
    assert proxy.sources == want
    assert len(want) == (0 if dtype == F16 else 2)      # p3 and p8
    plist = [params[k].detach() for k in names]
    for p, gw in zip(plist, glist):
        assert p.data_ptr() % 16 == 0 and p.is_contiguous()
        assert torch.equal(p, gw.unsqueeze(0).expand(C, *gw.shape))

    # 3. three SGD / FedProx steps on given gradients; client c's are
    # scaled by 0.5 + c/C so that the update norms spread
    spread = 0.5 + torch.arange(C, device="cuda", dtype=F32) / C
    lr32, mu32 = kb._f32(LR), kb._f32(mu)
    g64 = [kb.upcast(gw).reshape(-1) for gw in glist]
    before = [kb.upcast(p) for p in plist]
    for step in range(3):
        grads = [(0.1 * torch.randn(p.shape, generator=g, device="cuda")
                  * spread.view(-1, *[1] * (p.dim() - 1))).to(dtype)
                 for p in plist]
        fused.fused_sgd_update(plist, grads, lr=LR, mu=mu,
                               global_params=glist)
        after = [kb.upcast(p) for p in plist]
        for i, (a, b, gr) in enumerate(zip(after, before, grads)):
            n = glist[i].numel()
            ref, scale = kb.sgd_math(
                b.reshape(-1), kb.upcast(gr).reshape(-1), g64[i], [0, n], C,
                lr32, mu32)
            # w - lr*(g + mu*(w - m)): 4 roundings before the store
            kb.assert_bounded(a.reshape(-1), ref, scale, 4, dtype,
                              label=f"tail.sgd.{tag}")
        before = after

    # 4. squared update norms over all parameters
    finals = before
    sq = fused.client_delta_sqnorm(plist, glist)
    sq_ref = sum(((f.reshape(C, -1) - m) ** 2).sum(1)
                 for f, m in zip(finals, g64))
    P = master.numel()
    # as test_clip_gpu: every term non-negative, scale = ref; per
    # parameter the subtraction, the square and the += round once each
    kb.assert_bounded(sq, sq_ref, sq_ref, P + 4 * len(glist), F32,
                      label=f"tail.sq.{tag}")

    # 5. clip at S between the 3rd and 4th smallest fp64 norm: both sides
    # populated.  Checked, like test_clip_weights_bounded, from the sq the
    # kernel received, so no decision depends on fp32 against fp64.
    order = sq_ref.sort().values
    S = kb._f32(float(((order[2] + order[3]) / 2).sqrt()))
    weights = torch.rand(C, generator=g, device="cuda")
    weights[1::3] = 0.0
    w_eff, wsum = fused.clip_weights(sq, weights, S)
    q = kb.upcast(sq)
    s = torch.where(q > S * S, S / q.sqrt(), torch.ones_like(q))
    assert 3 <= int((s < 1).sum()) <= C - 3
    w_ref = kb.upcast(weights) * s
    kb.assert_bounded(w_eff, w_ref, w_ref.abs(), 1, F32, intrinsic=True,
                      label=f"tail.w_eff.{tag}")
    we = kb.upcast(w_eff)
    assert abs(float(kb.upcast(wsum)) - float(we.sum())) \
        <= (C + 2) * 2.0 ** -23 * float(we.abs().sum())

    # 6. accumulate into views of a non-zero flat delta
    delta_flat = torch.randn(P, generator=g, device="cuda")
    delta0 = kb.upcast(delta_flat)
    dviews = [master.views_of(delta_flat)[k] for k in names]
    for i, (dl, cw, gw) in enumerate(zip(dviews, plist, glist)):
        if_aligned, taken = ROUTES[(dtype, C)][i]
        n = gw.numel()
        assert dl.data_ptr() % 4 == 0
        assert ops.delta_accum_route(1, n, C, CODE[dtype], True, True) \
            == if_aligned, names[i]
        assert ops.delta_accum_route(
            1, n, C, CODE[dtype], gw.data_ptr() % 16 == 0,
            cw.data_ptr() % 16 == 0) == taken, names[i]
    fused.weighted_delta_accum(dviews, plist, glist, w_eff, wsum=wsum)
    for i, (f, m) in enumerate(zip(finals, g64)):
        n, off = m.numel(), OFFSETS[i]
        ref, _, scale_h = kb.delta_math(
            delta0[off:off + n], f.reshape(-1), m, we, [0, n], C,
            hoisted=True)
        # sum_c w_c buf_c - wsum*master + delta; wsum is itself an fp32
        # sum of the C weights: C more terms
        kb.assert_bounded(
            delta_flat[off:off + n], ref, scale_h, 2 * C + 1, F32,
            label=f"tail.accum.{tag}.{ROUTES[(dtype, C)][i][1]}")
