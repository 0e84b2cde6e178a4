"""conv3x3_wflip: w [C, OC, IC, 3, 3] -> wt [C, IC, OC, 3, 3] with the 9
taps reversed, against torch on the CPU.

It is data movement, so the comparison is on the raw 16-bit patterns and
exact.  The input is built from bit patterns, not values: element number
i of client c holds pattern (7 * i + 13 * c) mod 0x7F00, viewed as bf16
(all finite).  bf16 has fewer finite values than the larger cases have
elements, so a client's patterns repeat every 0x7F00 = 32512 elements (7
is coprime to it); closer than that every element differs from every
other, the smallest cases are distinct throughout, and a swapped tap (1..8
elements apart), a swapped channel (a small multiple of 9 or 9 * IC apart)
or a swapped client (13 * dc off at the same element) cannot pass."""

import pytest
import torch

pytestmark = pytest.mark.gpu

# (C, OC, IC)
CASES = [(1, 32, 32), (3, 64, 64), (2, 32, 96), (2, 96, 32), (2, 128, 64)]


@pytest.fixture(scope="module")
def ops():
    from olearning_sim_amd.ops import load_hip_ops
    return load_hip_ops(required=True)


def patterned_weight(C, OC, IC):
    n = OC * IC * 9
    i = torch.arange(n, dtype=torch.int64)[None, :]
    c = torch.arange(C, dtype=torch.int64)[:, None]
    bits = ((7 * i + 13 * c) % 0x7F00).to(torch.int16)
    return bits.view(torch.bfloat16).reshape(C, OC, IC, 3, 3).contiguous()


def reference_wflip(w_cpu):
    return w_cpu.flip(-1, -2).transpose(1, 2).contiguous()


@pytest.mark.parametrize("case", CASES, ids=str)
def test_wflip_matches_torch(ops, case):
    C, OC, IC = case
    w = patterned_weight(C, OC, IC)
    ref = reference_wflip(w)
    wt = ops.conv3x3_wflip(w.cuda())
    torch.cuda.synchronize()
    assert wt.shape == (C, IC, OC, 3, 3) and wt.is_contiguous()
    assert torch.equal(wt.cpu().view(torch.int16), ref.view(torch.int16))


def test_wflip_rejects_unsupported(ops):
    ok = patterned_weight(2, 32, 64).cuda()
    with pytest.raises(RuntimeError):          # OC not a multiple of 32
        ops.conv3x3_wflip(patterned_weight(1, 24, 32).cuda())
    with pytest.raises(RuntimeError):          # IC not a multiple of 32
        ops.conv3x3_wflip(patterned_weight(1, 32, 24).cuda())
    with pytest.raises(RuntimeError):          # non-contiguous
        ops.conv3x3_wflip(ok.transpose(1, 2))
    with pytest.raises(RuntimeError):          # fp32
        ops.conv3x3_wflip(ok.float())
    with pytest.raises(RuntimeError):          # 5x5 taps
        ops.conv3x3_wflip(torch.zeros(1, 32, 32, 5, 5, dtype=torch.bfloat16,
                                      device="cuda"))
