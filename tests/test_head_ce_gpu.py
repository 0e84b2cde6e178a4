"""The tied head's fused cross-entropy kernels (ops/csrc/head_ce.hip): both
kernels against fp64 on the exact bf16 tiles they read, their writes, the
route, and tied_head_ce on the fused route against kb.tied_head_math.

Bounds: items 2 to 4 of kb.assert_tied_head_bounded with d = 0, since the
tile is the kernel's exact input, and intrinsic=True (v_exp_f32, v_log_f32).
lse   sums V terms in fp32 (n = V); scale |max| + |lse - max| + 1 as for
      every log-sum-exp here.  E_lse is that bound.
zy    one fp32 addition of logit and bias (n = 1).
dl    g (p - onehot): p = exp(z - lse) moves by p expm1(E_lse); evaluated in
      fp32 over the V-term lse (n = V), one bf16 rounding of the perturbed
      value.  E_dl is the sum.
dbias sums N stored dlogits in fp32 (n = N), one bf16 rounding, and inherits
      the column sum of E_dl.
"""

import pytest
import torch

import kernel_bounds as kb

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
SENTINEL = 12345.678
PAD = 64
G = 1.0 / 24
LABELS_40 = [[0, 15, 16, 31, 32, 39, 7, 20], [39, 32, 31, 16, 15, 0, 33, 8]]
# (C, N, V, slice, variant).  The issue's six, then the column loops' second
# trips: stats chunks of 128 * VEC columns at VEC 8 (1032 = 1024 + 8), VEC 2
# (258 = 256 + 2) and VEC 1 (131 = 128 + 3).
CASES = [(2, 8, 40, 16, "plain"), (2, 5, 22, 16, "plain"),
         (2, 1, 21, 16, "plain"), (1, 4, 8, 8, "plain"),
         (2, 9, 520, 1024, "plain"), (2, 8, 40, 16, "shared_bias_far_max"),
         (2, 5, 2322, 1032, "plain"), (1, 2, 131, 256, "plain")]
_RUNS: dict = {}


def _place(shape, dtype):
    """An operand PAD elements into SENTINEL-filled storage, SENTINEL itself."""
    n = int(torch.Size(shape).numel())
    whole = torch.full((n + 2 * PAD,), SENTINEL, device="cuda", dtype=dtype)
    return whole[PAD:PAD + n].view(shape), whole


def _run(C, N, V, sv, variant):
    """The slice loop of stats, then of grad (out apart and out = logits)."""
    key = (C, N, V, sv, variant)
    if key in _RUNS:
        return _RUNS[key]
    from olearning_sim_amd.ops import head_ce
    gen = torch.Generator().manual_seed(C + 3 * N + 7 * V)
    slices = [(s0, min(s0 + sv, V)) for s0 in range(0, V, sv)]
    z = 2.0 * torch.randn(C, N, V, generator=gen)
    labels = torch.randint(0, V, (C, N), generator=gen)
    labels.view(-1)[0], labels.view(-1)[-1] = 0, V - 1
    if (N, V) == (8, 40):
        labels = torch.tensor(LABELS_40)
    if variant == "shared_bias_far_max":
        z[:, :, :sv] -= 80.0
        z[:, :, V - 3] += 6.0
        bias = (0.5 * torch.randn(V, generator=gen)).to(BF16).cuda() \
            .unsqueeze(0).expand(C, -1)
    else:
        bias = (0.5 * torch.randn(C, V, generator=gen)).to(BF16).cuda()
    tiles = [z[:, :, a:b].to(BF16).cuda().contiguous() for a, b in slices]
    labels = labels.cuda()
    out, whole = {}, {}
    for name, shape, dt in [("m", (C, N), F32), ("l", (C, N), F32),
                            ("zy", (C, N), F32), ("dbias", (C, V), BF16)] + \
            [(f"dl{i}", t.shape, BF16) for i, t in enumerate(tiles)]:
        out[name], whole[name] = _place(shape, dt)
    out["m"].fill_(float("-inf"))
    out["l"].zero_()
    out["zy"].zero_()
    for (s0, _), t in zip(slices, tiles):
        head_ce.head_ce_stats(t, bias, labels, s0, out["m"], out["l"],
                              out["zy"])
    dbias_alias = torch.empty_like(out["dbias"])
    alias = [t.clone() for t in tiles]
    for i, ((s0, _), t) in enumerate(zip(slices, tiles)):
        for src, dbias, dst in ((t, out["dbias"], out[f"dl{i}"]),
                                (alias[i], dbias_alias, alias[i])):
            assert head_ce.head_ce_grad(src, bias, labels, s0, out["m"],
                                        out["l"], G, dbias, out=dst) is dst
    torch.cuda.synchronize()
    _RUNS[key] = dict(out, whole=whole, tiles=tiles, bias=bias, labels=labels,
                      alias=alias, dbias_alias=dbias_alias)
    return _RUNS[key]


@pytest.mark.parametrize("C,N,V,sv,variant", CASES)
def test_kernels_against_fp64(C, N, V, sv, variant):
    r = _run(C, N, V, sv, variant)
    label = f"head_ce.{C}.{N}.{V}.{sv}.{variant}"
    u = kb.U_OUT[BF16]
    z0, b = torch.cat([kb.upcast(t) for t in r["tiles"]], dim=2), \
        kb.upcast(r["bias"]).unsqueeze(1)
    z, lab = z0 + b, r["labels"].cpu().unsqueeze(2)
    mx = z.amax(dim=2, keepdim=True)
    lse = z.logsumexp(dim=2, keepdim=True)
    lse_scale = mx.abs() + (lse - mx).abs() + 1.0
    kb.assert_bounded((r["m"] + torch.log(r["l"])).unsqueeze(2), lse,
                      lse_scale, V, F32, intrinsic=True, label=label + ".lse")
    kb.assert_bounded(r["zy"].unsqueeze(2), z.gather(2, lab),
                      (z0.abs() + b.abs()).gather(2, lab), 1, F32,
                      label=label + ".zy")
    e_lse = kb.bound(lse, lse_scale, V, F32, intrinsic=True)
    p = (z - lse).exp()
    onehot = torch.zeros_like(p).scatter_(2, lab, 1.0)
    dl, dl_scale = G * (p - onehot), G * (p + onehot)
    dp = (1 + u) * G * p * torch.expm1(e_lse)
    got = torch.cat([r[f"dl{i}"] for i in range(len(r["tiles"]))], dim=2)
    kb.assert_bounded(got, dl, dl_scale, V, BF16, intrinsic=True,
                      label=label + ".dlogits", extra=dp)
    e_dl = kb.bound(dl, dl_scale, V, BF16, intrinsic=True) + dp
    kb.assert_bounded(r["dbias"], dl.sum(dim=1), dl_scale.sum(dim=1), N, BF16,
                      label=label + ".dbias", extra=e_dl.sum(dim=1))


@pytest.mark.parametrize("C,N,V,sv,variant", CASES)
def test_writes_and_aliasing(C, N, V, sv, variant):
    r = _run(C, N, V, sv, variant)
    for name, whole in r["whole"].items():
        sent = torch.full((PAD,), SENTINEL, device="cuda", dtype=whole.dtype)
        assert torch.equal(whole[:PAD], sent), (name, "head")
        assert torch.equal(whole[-PAD:], sent), (name, "tail")
    sent = torch.tensor(SENTINEL, device="cuda", dtype=BF16)
    for i, a in enumerate(r["alias"]):
        assert not bool((r[f"dl{i}"] == sent).any()), "dlogits not written"
        assert torch.equal(a, r[f"dl{i}"]), "out = logits differs"
    assert not bool((r["dbias"] == sent).any()), "dbias element not written"
    assert torch.equal(r["dbias_alias"], r["dbias"])


def test_route(monkeypatch):
    from olearning_sim_amd import ops

    def route(s, dtype=BF16, off=0, device="cuda"):
        tile = torch.zeros(6 * s + off, device=device, dtype=dtype)
        return ops.head_ce_route(tile[off:].view(2, 3, s))

    assert [route(s) for s in (16, 6, 5)] == ["fused8", "fused2", "fused1"]
    assert route(16, dtype=F32) == "torch"
    assert route(16, device="cpu") == "torch"
    assert route(16, off=1) == "torch"
    assert route(16).startswith("fused")
    monkeypatch.setenv("OLSIM_HEAD_CE", "torch")
    assert route(16) == "torch"


@pytest.mark.parametrize("V", [40, 22])
def test_tied_head_ce_on_the_fused_route(V, monkeypatch):
    from olearning_sim_amd.models.bert import _TiedHeadCE, tied_head_ce
    from olearning_sim_amd.ops import head_ce
    monkeypatch.setattr(_TiedHeadCE, "SLICE_V", 16)
    C, N, H = 2, 8, 16
    gen = torch.Generator().manual_seed(V)
    hs = torch.randn(C, N, H, generator=gen).to(BF16)
    tok = (torch.randn(C, V, H, generator=gen) * 0.5).to(BF16)
    bias = (torch.randn(C, V, generator=gen) * 0.5).to(BF16)
    labels = torch.randint(0, V, (C, N), generator=gen)

    def run():
        before = head_ce.HEAD_CE_CALLS
        leaves = [t.cuda().requires_grad_(True) for t in (hs, tok, bias)]
        loss = tied_head_ce(*leaves, labels.cuda())
        loss.backward()
        return head_ce.HEAD_CE_CALLS - before, dict(
            zip(("dhs", "dtok", "dbias"), (t.grad for t in leaves)),
            loss=loss.detach())

    calls, got = run()
    assert calls == 2 * ((V + 15) // 16)
    up = kb.upcast
    ref = kb.tied_head_math(up(hs), up(tok), up(bias), labels, 16)
    kb.assert_tied_head_bounded(got, ref, up(hs), up(tok), BF16, 16,
                                label=f"tied.fused.V{V}")
    monkeypatch.setenv("OLSIM_HEAD_CE", "torch")
    assert run()[0] == 0
