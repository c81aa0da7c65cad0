"""GPU: K1 (cost-volume build) through the C ABI vs the oracle and the reference's golden vectors.

Tolerances (fp32): the HIP kernel evaluates the same lerp / pooling / bilinear formulas with a
different summation order -> 2e-5 absolute on N(0,1)-scale features (observed ~2e-6); the
reference's own int-vs-sampled discrepancy is 3.8e-5.
"""
import numpy as np
import pytest
import torch

import oracle
import synth
from helpers import load, t

pytestmark = pytest.mark.gpu
ATOL = 2e-5


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.mark.parametrize("name", ["block_cost_int_0", "block_cost_int_1", "block_cost_int_2",
                                  "block_cost_int_scale1", "block_cost_int_scale2"])
def test_int_path_golden(name):
    import temporalstereo_amd as ts
    g = load(name)
    dev = _dev()
    out = ts.block_cost(t(g["left"], dev), t(g["right"], dev), int(g["num_disp"]), int(g["scales"]))
    assert tuple(out.shape) == g["out"].shape
    np.testing.assert_allclose(out.cpu().numpy(), g["out"], rtol=1e-5, atol=ATOL)


@pytest.mark.parametrize("name", ["block_cost_sampled_0", "block_cost_sampled_1", "block_cost_sampled_2",
                                  "block_cost_sampled_scale1", "block_cost_sampled_scale2"])
def test_sampled_path_golden(name):
    import temporalstereo_amd as ts
    g = load(name)
    dev = _dev()
    out = ts.block_cost(t(g["left"], dev), t(g["right"], dev), t(g["disp"], dev), int(g["scales"]))
    np.testing.assert_allclose(out.cpu().numpy(), g["out"], rtol=1e-5, atol=ATOL)


def test_value_test_known_answer():
    """Reference-authored 3x4 value test needs H,W>=4 here, so embed it in a 4x4 frame: candidate d
    of the warped half must read right[x-d] exactly (integers are exactly representable)."""
    import temporalstereo_amd as ts
    dev = _dev()
    H, W = 4, 4
    left = torch.arange(1, H * W + 1, dtype=torch.float32).reshape(1, 1, H, W).repeat(1, 8, 1, 1).to(dev)
    right = (left + H * W).contiguous()
    ds = torch.linspace(-2, 2, 5).view(1, 5, 1, 1).expand(1, 5, H, W).contiguous().to(dev)
    out = ts.block_cost(left, right, ds, 3)
    warped = out[0, 8].cpu().numpy()        # first warped channel [D,H,W]
    R = right[0, 0].cpu().numpy()
    for k, d in enumerate(range(-2, 3)):
        exp = np.zeros_like(R)
        for x in range(W):
            if 0 <= x - d < W:
                exp[:, x] = R[:, x - d]
        np.testing.assert_allclose(warped[k], exp, atol=1e-4)
    np.testing.assert_array_equal(out[0, :8].cpu().numpy(), left[0].unsqueeze(1).expand(8, 5, H, W).cpu().numpy())


SHAPES = [  # B, C, H, W, D  -- levels of the BASELINE configs at reduced batch/channels + ragged sizes
    (1, 32, 34, 60, 12),     # config 2 coarse geometry (H not a multiple of 4)
    (1, 16, 68, 120, 5),     # config 2 fine geometry
    (2, 16, 24, 78, 12),     # KITTI 1/16: W % 4 != 0 -> scalar path
    (1, 8, 30, 40, 8),       # TartanAir 1/16
    (1, 8, 7, 9, 3),         # tiny ragged
    (1, 8, 4, 4, 2),         # minimum
    (1, 8, 12, 600, 3),      # row wider than the LDS staging limit -> global gather path
    (1, 16, 12, 38, 5),      # ragged width with THREE left quads per thread and row pair: runs as the four-row form (round 5: its LDS was
    (1, 16, 12, 78, 3),      # sized for the two-row form and every correlation plane came out wrong; no BASELINE geometry is ragged)
]


MANY_PLANES = [  # B * C/8 * D = 65,600 planes of the pooled maps, more than one grid dimension holds: the expansion folds them over
    (4, 128, 4, 8, 1025),    # two.  Aligned.                          (Several passes of items per workgroup: block_cost_main.)
    (4, 128, 5, 9, 1025),    # ragged: scalar loads and stores, H not a multiple of 4
]


@pytest.mark.parametrize("shape", SHAPES + MANY_PLANES)
def test_int_path_vs_oracle(shape):
    import temporalstereo_amd as ts
    B, C, H, W, D = shape
    dev = _dev()
    L = synth.normal(7, "L", (B, C, H, W)); R = synth.normal(7, "R", (B, C, H, W))
    exp = oracle.block_cost(t(L), t(R), D, 3)
    got = ts.block_cost(t(L, dev), t(R, dev), D, 3).cpu()
    np.testing.assert_allclose(got.numpy(), exp.numpy(), rtol=1e-5, atol=ATOL)


@pytest.mark.parametrize("shape", SHAPES)
def test_sampled_path_vs_oracle(shape):
    import temporalstereo_amd as ts
    B, C, H, W, D = shape
    D = max(D, 2)
    dev = _dev()
    L = synth.normal(8, "L", (B, C, H, W)); R = synth.normal(8, "R", (B, C, H, W))
    disp = synth.uniform(8, "d", (B, D, H, W), -4.0, min(W, 40) + 2.0)
    disp[:, 0] = np.round(disp[:, 0])
    exp = oracle.block_cost(t(L), t(R), t(disp), 3)
    got = ts.block_cost(t(L, dev), t(R, dev), t(disp, dev), 3).cpu()
    np.testing.assert_allclose(got.numpy(), exp.numpy(), rtol=1e-5, atol=ATOL)


def test_sampled_equals_int_at_integer_candidates():
    """Size-independent property at the FULL config-2 coarse size: integer candidates through the
    sampled path reproduce the int path's target volume (cost = -(L - warped)^2)."""
    import temporalstereo_amd as ts
    dev = _dev()
    B, C, H, W, D = 1, 256, 34, 60, 12
    L = t(synth.normal(9, "L", (B, C, H, W)), dev); R = t(synth.normal(9, "R", (B, C, H, W)), dev)
    ci = ts.block_cost(L, R, D, 3)
    ds = torch.arange(D, dtype=torch.float32, device=dev).view(1, D, 1, 1).expand(B, D, H, W).contiguous()
    cs = ts.block_cost(L, R, ds, 3)
    np.testing.assert_allclose((-(cs[:, :C] - cs[:, C:2 * C]) ** 2).cpu().numpy(), ci[:, :C].cpu().numpy(), atol=1e-4)
    np.testing.assert_allclose(cs[:, 2 * C:].cpu().numpy(), ci[:, C:].cpu().numpy(), rtol=2e-5, atol=1e-4)


def test_full_size_precise_level_properties():
    """BASELINE config 2 precise level [1,128,136,240] D=5: reference half is an exact broadcast,
    zero disparity reproduces the right map exactly, group-0 block equals -sum_8 (L-t)^2."""
    import temporalstereo_amd as ts
    dev = _dev()
    B, C, H, W, D = 1, 128, 136, 240, 5
    L = t(synth.normal(10, "L", (B, C, H, W)), dev); R = t(synth.normal(10, "R", (B, C, H, W)), dev)
    disp = t(synth.uniform(10, "d", (B, D, H, W), 0.0, 48.0), dev)
    disp[:, 2] = 0.0
    out = ts.block_cost(L, R, disp, 3)
    assert out.shape == (B, 2 * C + 3 * C // 8, D, H, W)
    assert torch.equal(out[:, :C], L.unsqueeze(2).expand(B, C, D, H, W))
    # zero shift: the reference's coordinate round trip is not exactly the identity (Appendix B.1)
    np.testing.assert_allclose(out[:, C:2 * C, 2].cpu().numpy(), R.cpu().numpy(), atol=1e-4)
    e = out[:, :C] - out[:, C:2 * C]
    g0 = -(e * e).view(B, C // 8, 8, D, H, W).sum(2)
    np.testing.assert_allclose(out[:, 2 * C:2 * C + C // 8].cpu().numpy(), g0.cpu().numpy(), rtol=1e-5, atol=1e-4)
    assert torch.isfinite(out).all()


@pytest.mark.parametrize("sampled", [False, True])
@pytest.mark.parametrize("shape", [(2, 16, 10, 14, 3), (1, 8, 9, 13, 4), (1, 16, 12, 20, 5), (2, 24, 21, 130, 3), (1, 8, 7, 258, 2),
                                   (1, 16, 34, 60, 8), (1, 8, 8, 520, 2),     # more items than the tile kernel takes
                                   (1, 16, 9, 312, 5), (2, 8, 6, 512, 3)])     # the 512-lane form of the row kernels (KITTI's 1/4 level is 312 wide)
def test_backward_vs_oracle_autograd(shape, sampled):
    """Gradients through the C ABI backward vs autograd of the oracle (same torch ops as the
    reference).  fp32 atomics -> 1e-4 relative to the gradient scale."""
    import temporalstereo_amd as ts
    B, C, H, W, D = shape
    dev = _dev()
    L = synth.normal(11, "L", (B, C, H, W)); R = synth.normal(11, "R", (B, C, H, W))
    disp = synth.uniform(11, "d", (B, D, H, W), -2.0, W + 1.0)
    ctot = (2 * C if sampled else C) + 3 * C // 8
    gout = synth.normal(11, "g", (B, ctot, D, H, W))

    lc, rc, dc = t(L).requires_grad_(), t(R).requires_grad_(), t(disp).requires_grad_()
    ref = oracle.block_cost(lc, rc, dc if sampled else D, 3)
    ref.backward(t(gout))

    lg, rg, dg = t(L, dev).requires_grad_(), t(R, dev).requires_grad_(), t(disp, dev).requires_grad_()
    out = ts.block_cost(lg, rg, dg if sampled else D, 3)
    out.backward(t(gout, dev))

    def close(a, b, what):
        scale = float(b.abs().max()) + 1e-6
        err = float((a.cpu() - b).abs().max())
        assert err <= 2e-4 * scale + 1e-5, "%s: max err %g (scale %g)" % (what, err, scale)
    close(lg.grad, lc.grad, "grad_left")
    close(rg.grad, rc.grad, "grad_right")
    if sampled:
        close(dg.grad, dc.grad, "grad_disp")


@pytest.mark.parametrize("shape", [(1, 16, 20, 36, 5), (2, 32, 34, 60, 7), (1, 128, 68, 120, 5), (1, 64, 135, 240, 5),
                                   (3, 8, 9, 256, 3), (1, 16, 12, 260, 5), (1, 16, 12, 38, 5), (1, 8, 4, 4, 2), (1, 16, 9, 312, 5), (1, 8, 6, 512, 3)])
@pytest.mark.parametrize("scales", [3, 2])
def test_correlation_blocks_alone_equal_the_full_op(shape, scales):
    """ts_block_cost_sampled_corr_fwd (what the pipeline launches: block_cost_corr_rows on aligned maps of up to 256 columns,
    block_cost_fast<corr only> otherwise -- W = 260 and the ragged W = 38 here) against the complete op's correlation channels
    (block_cost.py:66-81) and against the oracle, within the op's tolerance.  Candidates reach outside the row on both
    sides; H is not always a multiple of 4."""
    import temporalstereo_amd as ts
    import temporalstereo_amd.functional as TF
    dev = _dev()
    B, C, H, W, D = shape
    L = t(synth.normal(11, "L", (B, C, H, W)), dev)
    R = t(synth.normal(11, "R", (B, C, H, W)), dev)
    disp = t(synth.uniform(11, "d", (B, D, H, W), -3.0, 0.6 * W), dev)
    corr = TF.block_cost_corr(L, R, disp, scales)
    full = ts.block_cost(L, R, disp, scales)
    assert corr.shape == (B, scales * (C // 8), D, H, W)
    # (the two launches are different instantiations: contraction of multiply-adds may differ in the last bits; bit-identity of
    # block_cost_corr_rows with block_cost_fast<corr only> is recorded in profiles/r05_k1_corr_rows.txt)
    np.testing.assert_allclose(corr.cpu().numpy(), full[:, 2 * C:].cpu().numpy(), rtol=1e-5, atol=ATOL)
    exp = oracle.block_cost(L.cpu(), R.cpu(), disp.cpu(), scales)[:, 2 * C:]
    np.testing.assert_allclose(corr.cpu().numpy(), exp.numpy(), rtol=5e-5, atol=ATOL * max(1.0, C / 16.0))
