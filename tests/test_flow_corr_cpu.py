"""tests/flow_corr_ref.py (the closed form of FlowCorrBlock that the HIP kernels implement and the GPU tests expect) pinned to the
reference's own runs recorded in tests/golden/flow_corr_*.npz (tools/gen_golden.py --only-flow).  No GPU.

The fixtures hold the reference's fp32 results and how far they lie from its fp64 run (dev_*, rel_grad_*).  The restatement in fp64
stands where the reference's fp64 run stands, so it must lie within the same distance of the stored fp32 values, up to the factor 2
that the `.float()` of the stored values and a one-ulp disagreement on the maximum may add; the restatement in fp32 is a second,
equally rounded evaluation and may land twice as far from fp64 as the first, hence 4 (the argument of tests/test_raft_corr_gpu.py):
  pyramid, output   |flow_corr_ref fp64 - stored fp32| <= 2 dev      |flow_corr_ref fp32 - flow_corr_ref fp64| <= 4 dev
  gradients         relative L2 (fp64 autograd, stored fp32) <= 2 rel_grad      relative L2 (fp32 autograd, fp64 autograd) <= 4 rel_grad
"""
import pytest
import torch

import flow_corr_ref as R

TAGS = ("a", "c", "e")
SHAPES = {"a": (2, 6, 8, 11, 3, 2), "c": (1, 40, 4, 4, 2, 1), "e": (1, 32, 8, 16, 3, 3)}
GRADS = ("fmap1", "fmap2", "coords")


def tensors(tag, dtype):
    g = R.load_fixture(tag)
    return g, tuple(torch.from_numpy(g[k]).to(dtype) for k in GRADS)


@pytest.mark.parametrize("tag", TAGS)
def test_fixture_is_the_listed_shape(tag):
    g, (f1, f2, c) = tensors(tag, torch.float32)
    B, C, H, W, L, r = SHAPES[tag]
    assert tuple(f1.shape) == tuple(f2.shape) == (B, C, H, W) and tuple(c.shape) == (B, 2, H, W)
    assert (int(g["num_levels"]), int(g["radius"])) == (L, r)
    assert tuple(g["out"].shape) == tuple(g["cot"].shape) == (B, L * (2 * r + 1) ** 2, H, W)
    nz = float((g["out"] != 0).mean())
    assert 0.4 <= nz <= 0.95
    import temporalstereo_amd as ts
    flow = c - ts.FlowCorrBlock.init_flow((B, C, H, W), "cpu")[0]
    assert float(flow[:, 0].abs().max()) <= 0.25 * W + 1e-4 and float(flow[:, 1].abs().max()) <= 0.25 * H + 1e-4


@pytest.mark.parametrize("tag", TAGS)
def test_pyramid_and_output_against_the_reference(tag):
    g, (f1, f2, c) = tensors(tag, torch.float64)
    B, C, H, W, L, r = SHAPES[tag]
    levels = R.corr_pyramid(f1, f2, L)
    levels32 = R.corr_pyramid(f1.float(), f2.float(), L)
    for i, P in enumerate(levels):
        stored = torch.from_numpy(g["pyr_%d" % i]).double()
        dev = float(g["dev_pyr_%d" % i])
        assert tuple(stored.shape) == (B * H * W, (H >> i) * (W >> i))
        err = float((P.reshape(stored.shape) - stored).abs().max())
        assert err <= 2 * dev, (i, err, dev)
        err32 = float((levels32[i].double() - P).abs().max())
        assert err32 <= 4 * dev, (i, err32, dev)
    out = R.lookup(levels, c, r)
    err = float((out - torch.from_numpy(g["out"]).double()).abs().max())
    assert err <= 2 * float(g["dev_out"]), (err, float(g["dev_out"]))
    err32 = float((R.lookup(levels32, c.float(), r).double() - out).abs().max())
    assert err32 <= 4 * float(g["dev_out"]), (err32, float(g["dev_out"]))


@pytest.mark.parametrize("tag", TAGS)
def test_gradients_against_the_reference(tag):
    B, C, H, W, L, r = SHAPES[tag]
    grads = {}
    for dt in (torch.float64, torch.float32):
        g, ins = tensors(tag, dt)
        f1, f2, c = (t.requires_grad_(True) for t in ins)
        R.flow_corr_block(f1, f2, c, L, r).backward(torch.from_numpy(g["cot"]).to(dt))
        grads[dt] = (f1.grad, f2.grad, c.grad)
    for name, g64, g32 in zip(GRADS, grads[torch.float64], grads[torch.float32]):
        stored = torch.from_numpy(g["grad_" + name]).double()
        rel = float((g64 - stored).norm() / g64.norm())
        assert rel <= 2 * float(g["rel_grad_" + name]), (name, rel, float(g["rel_grad_" + name]))
        rel32 = float((g32.double() - g64).norm() / g64.norm())
        assert rel32 <= 4 * float(g["rel_grad_" + name]), (name, rel32, float(g["rel_grad_" + name]))


def test_positions_keep_off_the_kinks():
    """the generator's rule, checked on what it stored: no position within 1e-3 of an integer, fp32 and fp64 floors equal"""
    for tag in TAGS:
        g, (_, _, c) = tensors(tag, torch.float32)
        B, C, H, W, L, r = SHAPES[tag]
        for i in range(L):
            for a64, a32 in zip(R.positions(c.double(), i, r, H >> i, W >> i), R.positions(c, i, r, H >> i, W >> i)):
                assert float((a64 - torch.round(a64)).abs().min()) >= 1e-3
                assert torch.equal(torch.floor(a64), torch.floor(a32.double()))


def test_restatement_refuses_an_empty_level():
    with pytest.raises(ValueError):
        R.corr_pyramid(torch.zeros(1, 2, 3, 8), torch.zeros(1, 2, 3, 8), 3)
    assert tuple(R.corr_pyramid(torch.zeros(1, 2, 4, 9), torch.zeros(1, 2, 4, 9), 3)[-1].shape) == (1, 36, 1, 2)


def test_init_flow_is_the_pixel_grid():
    import temporalstereo_amd as ts
    ref, tgt = ts.FlowCorrBlock.init_flow((2, 5, 3, 4), "cpu")
    assert tuple(ref.shape) == (2, 2, 3, 4) and ref.dtype == torch.float32 and torch.equal(ref, tgt)
    assert torch.equal(ref[1, 0], torch.arange(4.0).view(1, 4).expand(3, 4)) and torch.equal(ref[0, 1], torch.arange(3.0).view(3, 1).expand(3, 4))
    flow = torch.full((2, 2, 3, 4), 0.5)
    ref, tgt = ts.FlowCorrBlock.init_flow((2, 5, 3, 4), "cpu", flow_init=flow)
    assert torch.equal(tgt, ref + 0.5)
    with pytest.raises(ValueError, match="init_flow"):
        ts.FlowCorrBlock.init_flow((2, 3, 4), "cpu")


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    """the wrapper's refusals that need no GPU: they come before any launch"""
    import temporalstereo_amd as ts
    f = torch.zeros(1, 4, 16, 16)
    c = torch.zeros(1, 2, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ts.FlowCorrBlock(f, f)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ts.flow_corr_lookup(torch.zeros(256 * 256), c, 1)
    with pytest.raises(ValueError, match=r"must be \[B,C,H,W\]"):
        ts.flow_corr_pyramid(f[0], f[0], 1)
    with pytest.raises(ValueError, match="differ in shape"):
        ts.flow_corr_pyramid(f, torch.zeros(1, 4, 16, 15), 2)
    with pytest.raises(ValueError, match="num_levels must be >= 1"):
        ts.flow_corr_pyramid(f, f, 0)
    with pytest.raises(ValueError, match="pools at most 4 levels"):
        ts.FlowCorrBlock(torch.zeros(1, 4, 64, 64), torch.zeros(1, 4, 64, 64), num_levels=5)
    with pytest.raises(ValueError, match="level 2 of a 7 x 16 map is 1 x 4"):
        ts.FlowCorrBlock(torch.zeros(1, 4, 7, 16), torch.zeros(1, 4, 7, 16), num_levels=3)
    with pytest.raises(ValueError, match="level 0 of a 8 x 1 map"):
        ts.flow_corr_pyramid(torch.zeros(1, 4, 8, 1), torch.zeros(1, 4, 8, 1), 1)
    with pytest.raises(ValueError, match="radius must be >= 0"):
        ts.FlowCorrBlock(f, f, radius=-1)
    with pytest.raises(ValueError, match="radius must be >= 0"):
        ts.flow_corr_lookup(torch.zeros(256 * 256), c, -1)
    with pytest.raises(ValueError, match=r"coords must be \[B,2,H,W\]"):
        ts.flow_corr_lookup(torch.zeros(256 * 256), c[:, :1], 1)
    with pytest.raises(ValueError, match="does not match size"):
        ts.flow_corr_lookup(torch.zeros(256 * 256), c, 1, size=(16, 15))


def test_pyramid_buffer_length_decides_the_level_count():
    from temporalstereo_amd import functional as Fn
    N, H, W = 2 * 8 * 16, 8, 16
    assert Fn._FLOW.levels_of(torch.zeros(N * 128), N, H, W) == 1
    assert Fn._FLOW.levels_of(torch.zeros(N * (128 + 32 + 8)), N, H, W) == 3
    with pytest.raises(ValueError, match="no pyramid of a 8 x 16 map"):
        Fn._FLOW.levels_of(torch.zeros(N * (128 + 32 + 8 + 2)), N, H, W)       # a fourth level would be 1 x 2
    with pytest.raises(ValueError, match="no pyramid of a 8 x 16 map"):
        Fn._FLOW.levels_of(torch.zeros(N * 127), N, H, W)
    with pytest.raises(ValueError, match="1-D buffer"):
        Fn._FLOW.levels_of(torch.zeros(N * 128 + 1), N, H, W)
    views = Fn.flow_corr_level_views(torch.zeros(N * (128 + 32 + 8)), 2, H, W, 3)
    assert [tuple(v.shape) for v in views] == [(N, 1, 8, 16), (N, 1, 4, 8), (N, 1, 2, 4)]


def test_entries_refuse_bad_sizes_without_gpu():
    """the library's own checks (before any launch): the statuses and messages of include/ts_hip.h"""
    from temporalstereo_amd import _lib
    L = _lib.lib()
    one = 16        # any non-null pointer: a refused call dereferences nothing
    assert L.ts_flow_corr_pyramid_fwd(one, one, one, 1, 4, 7, 16, 3, None) == -2 and b"level 2" in L.ts_last_error_string()
    assert L.ts_flow_corr_pyramid_fwd(one, one, one, 1, 4, 8, 1, 1, None) == -2 and b"level 0" in L.ts_last_error_string()
    assert L.ts_flow_corr_pyramid_fwd(one, one, one, 1, 4, 8, 16, 0, None) == -2 and b"num_levels" in L.ts_last_error_string()
    assert L.ts_flow_corr_pyramid_fwd(one, one, one, 1, 4, 64, 64, 5, None) == -3 and b"at most 4 levels" in L.ts_last_error_string()
    assert L.ts_flow_corr_pyramid_fwd(one, None, one, 1, 4, 8, 16, 2, None) == -1 and b"NULL" in L.ts_last_error_string()
    assert L.ts_flow_corr_lookup_fwd(one, one, one, 1, 8, 16, 2, -1, None) == -2 and b"radius" in L.ts_last_error_string()
    assert L.ts_flow_corr_lookup_bwd(one, one, one, None, None, 1, 8, 16, 2, 1, 1, None) == -1
    assert L.ts_flow_corr_lookup_bwd(None, one, one, one, None, 1, 8, 16, 2, 1, 1, None) == -1        # grad_coords needs the pyramid
    assert L.ts_flow_corr_lookup_bwd(one, one, one, one, one, 1, 8, 16, 2, 40, 1, None) == -3 and b"LDS" in L.ts_last_error_string()
    assert L.ts_flow_corr_pyramid_bwd(one, one, one, None, None, 1, 4, 8, 16, 1, None) == -1
    assert L.ts_version() >= 16
