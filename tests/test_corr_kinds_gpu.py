"""CorrBlock and FlowCorrBlock in ONE autograd graph over shared feature maps.  The two blocks run through the same autograd Functions
(temporalstereo_amd/functional.py, `_CorrPyramid`, `_CorrLookup`, `_CorrBlockLookup`) and differ only in the kind these carry in their
ctx; tests/test_raft_corr_gpu.py and tests/test_flow_corr_gpu.py run one kind at a time and cannot see a kind that reaches the wrong
backward, or a gradient returned in another input's slot.

Bar: bit-equality.  Both backwards are bit-reproducible (asserted in the two files named above), the gradient of a shared leaf is the
fp32 sum of two terms, and such a sum does not depend on the order of its terms: so the feature gradients of the joint graph are, bit
for bit, the sum of those of the two blocks run alone on fresh leaves, and the gradients of disp and coords are those of their own block.

Shape [2,5,4,6], num_levels = 2, radius = 1: the smallest legal for both kinds (6 -> 3 for the rows; 4 x 6 -> 2 x 3 for the maps)."""
import pytest
import torch

import temporalstereo_amd as ts
from compare import same_bits

pytestmark = pytest.mark.gpu

B, C, H, W, L, RAD = 2, 5, 4, 6, 2, 1


def inputs():
    g = torch.Generator().manual_seed(20)
    f1, f2 = torch.randn(B, C, H, W, generator=g), torch.randn(B, C, H, W, generator=g)
    disp = torch.rand(B, 1, H, W, generator=g) * 4.0 - 1.0                                              # up to 3 cells left, 1 right
    coords = ts.FlowCorrBlock.init_flow((B, C, H, W), "cpu")[1] + (torch.rand(B, 2, H, W, generator=g) * 3.0 - 1.5)
    cot_r = torch.randint(-8, 9, (B, L * (2 * RAD + 1), H, W), generator=g).float() / 8
    cot_f = torch.randint(-8, 9, (B, L * (2 * RAD + 1) ** 2, H, W), generator=g).float() / 8
    dev = torch.device("cuda", torch.cuda.current_device())
    return tuple(t.to(dev) for t in (f1, f2, disp, coords, cot_r, cot_f))


def raft_out(composed, f1, f2, disp):
    if composed == "block":
        return ts.CorrBlock(f1, f2, L, RAD)(disp)
    return ts.raft_corr_lookup(ts.raft_corr_pyramid(f1, f2, L), disp, RAD)


def flow_out(composed, f1, f2, coords):
    if composed == "block":
        return ts.FlowCorrBlock(f1, f2, L, RAD)(coords)
    return ts.flow_corr_lookup(ts.flow_corr_pyramid(f1, f2, L), coords, RAD)


@pytest.mark.parametrize("composed", ("block", "functional"))
def test_both_kinds_in_one_graph(composed):
    f1, f2, disp, coords, cot_r, cot_f = inputs()

    def alone(fn, motion, cot):
        a, b, m = (t.clone().requires_grad_(True) for t in (f1, f2, motion))
        fn(composed, a, b, m).backward(cot)
        return a.grad, b.grad, m.grad
    r1, r2, rd = alone(raft_out, disp, cot_r)
    w1, w2, wc = alone(flow_out, coords, cot_f)
    for t in (r1, r2, rd, w1, w2, wc):
        assert float(t.abs().max()) > 0                                          # every gradient is there to be misrouted
    assert not same_bits(r1, w1) and not same_bits(r2, w2)

    a, b, d, c = (t.clone().requires_grad_(True) for t in (f1, f2, disp, coords))
    torch.autograd.backward([raft_out(composed, a, b, d), flow_out(composed, a, b, c)], [cot_r, cot_f])
    assert same_bits(a.grad, r1 + w1) and same_bits(b.grad, r2 + w2)
    assert same_bits(d.grad, rd) and same_bits(c.grad, wc)
