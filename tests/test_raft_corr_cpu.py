"""tests/raft_ref.py (the closed form of CorrBlock that the HIP kernels implement and the GPU tests expect) pinned to the reference's own
runs recorded in tests/golden/raft_corr_*.npz (tools/gen_golden.py --only-raft).  No GPU.

The fixtures hold the reference's fp32 results and how far they lie from its fp64 run (dev_*, rel_grad_*).  The restatement in fp64
stands where the reference's fp64 run stands, so it must lie within the same distance of the stored fp32 values, up to the factor 2
that the `.float()` of the stored values and a one-ulp disagreement on the maximum may add:
  pyramid, output   |raft_ref fp64 - stored fp32| <= 2 dev
  gradients         relative L2 (raft_ref fp64 autograd, stored fp32) <= 2 rel_grad
"""
import pytest
import torch

import raft_ref as R

TAGS = ("a", "b", "c", "e")
SHAPES = {"a": (2, 6, 3, 37, 4, 4), "b": (1, 5, 2, 66, 4, 4), "c": (1, 40, 1, 8, 4, 1), "e": (1, 32, 4, 64, 3, 2)}


def tensors(tag, dtype):
    g = R.load_fixture(tag)
    return g, tuple(torch.from_numpy(g[k]).to(dtype) for k in ("fmap1", "fmap2", "disp"))


@pytest.mark.parametrize("tag", TAGS)
def test_fixture_is_the_listed_shape(tag):
    g, (f1, f2, d) = tensors(tag, torch.float32)
    B, C, H, W, L, r = SHAPES[tag]
    assert tuple(f1.shape) == tuple(f2.shape) == (B, C, H, W) and tuple(d.shape) == (B, 1, H, W)
    assert (int(g["num_levels"]), int(g["radius"])) == (L, r)
    assert tuple(g["out"].shape) == tuple(g["cot"].shape) == (B, L * (2 * r + 1), H, W)
    nz = float((g["out"] != 0).mean())
    assert 0.5 <= nz <= 0.95
    lo, hi = float(d.min()) / W, float(d.max()) / W
    assert -0.2 <= lo and hi <= 0.7


@pytest.mark.parametrize("tag", TAGS)
def test_pyramid_and_output_against_the_reference(tag):
    g, (f1, f2, d) = tensors(tag, torch.float64)
    B, C, H, W, L, r = SHAPES[tag]
    levels = R.corr_pyramid(f1, f2, L)
    for i, P in enumerate(levels):
        stored = torch.from_numpy(g["pyr_%d" % i]).double()
        assert tuple(stored.shape) == (B * H * W, W >> i)
        err = float((P.reshape(stored.shape) - stored).abs().max())
        assert err <= 2 * float(g["dev_pyr_%d" % i]), (i, err, float(g["dev_pyr_%d" % i]))
    out = R.lookup(levels, d, r)
    err = float((out - torch.from_numpy(g["out"]).double()).abs().max())
    assert err <= 2 * float(g["dev_out"]), (err, float(g["dev_out"]))


@pytest.mark.parametrize("tag", TAGS)
def test_gradients_against_the_reference(tag):
    g, ins = tensors(tag, torch.float64)
    B, C, H, W, L, r = SHAPES[tag]
    f1, f2, d = (t.requires_grad_(True) for t in ins)
    R.corr_block(f1, f2, d, L, r).backward(torch.from_numpy(g["cot"]).double())
    for name, t in (("fmap1", f1), ("fmap2", f2), ("disp", d)):
        stored = torch.from_numpy(g["grad_" + name]).double()
        rel = float((t.grad - stored).norm() / t.grad.norm())
        assert rel <= 2 * float(g["rel_grad_" + name]), (name, rel, float(g["rel_grad_" + name]))


def test_positions_keep_off_the_kinks():
    """the generator's rule, checked on what it stored: no position within 1e-3 of an integer, fp32 and fp64 floors equal"""
    for tag in TAGS:
        g, (_, _, d) = tensors(tag, torch.float32)
        B, C, H, W, L, r = SHAPES[tag]
        for i in range(L):
            x64, x32 = R.positions(d.double(), i, r, W >> i), R.positions(d, i, r, W >> i)
            assert float((x64 - torch.round(x64)).abs().min()) >= 1e-3
            assert torch.equal(torch.floor(x64), torch.floor(x32.double()))


def test_restatement_refuses_an_empty_level():
    with pytest.raises(ValueError):
        R.corr_pyramid(torch.zeros(1, 2, 1, 7), torch.zeros(1, 2, 1, 7), 4)
    assert R.corr_pyramid(torch.zeros(1, 2, 1, 8), torch.zeros(1, 2, 1, 8), 4)[-1].shape[-1] == 1


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    """the wrapper's refusals that need no GPU: they come before any launch"""
    import temporalstereo_amd as ts
    f = torch.zeros(1, 4, 2, 16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ts.CorrBlock(f, f)
    with pytest.raises(ValueError, match="too narrow"):
        ts.CorrBlock(torch.zeros(1, 4, 2, 7), torch.zeros(1, 4, 2, 7), num_levels=4)
    with pytest.raises(ValueError, match="W >= 2"):
        ts.raft_corr_pyramid(torch.zeros(1, 4, 2, 1), torch.zeros(1, 4, 2, 1), 1)
    with pytest.raises(ValueError, match="num_levels must be >= 1"):
        ts.raft_corr_pyramid(f, f, 0)
    with pytest.raises(ValueError, match="differ in shape"):
        ts.raft_corr_pyramid(f, torch.zeros(1, 4, 2, 15), 2)


def test_pyramid_buffer_length_decides_the_level_count():
    from temporalstereo_amd import functional as Fn
    N, H, W = 2 * 2 * 16, 2, 16
    assert Fn._RAFT.levels_of(torch.zeros(N * 16), N, H, W) == 1
    assert Fn._RAFT.levels_of(torch.zeros(N * (16 + 8 + 4)), N, H, W) == 3
    assert Fn._RAFT.levels_of(torch.zeros(N * (16 + 8 + 4 + 2 + 1)), N, H, W) == 5      # a sixth level would be empty and adds nothing
    with pytest.raises(ValueError, match="no pyramid of width 16"):
        Fn._RAFT.levels_of(torch.zeros(N * 32), N, H, W)
    with pytest.raises(ValueError, match="no pyramid of width 16"):
        Fn._RAFT.levels_of(torch.zeros(N * 15), N, H, W)
    with pytest.raises(ValueError, match="1-D buffer"):
        Fn._RAFT.levels_of(torch.zeros(N * 16 + 1), N, H, W)
    views = Fn.raft_corr_level_views(torch.zeros(N * (16 + 8 + 4)), 2, H, W, 3)
    assert [tuple(v.shape) for v in views] == [(N, 1, 1, 16), (N, 1, 1, 8), (N, 1, 1, 4)]


def test_entries_refuse_bad_sizes_without_gpu():
    """the library's own checks (before any launch): the statuses and messages of include/ts_hip.h"""
    from temporalstereo_amd import _lib
    L = _lib.lib()
    one = 16        # any non-null pointer: a refused call dereferences nothing
    assert L.ts_raft_corr_pyramid_fwd(one, one, one, 1, 4, 2, 7, 4, None) == -2 and b"too narrow" in L.ts_last_error_string()
    assert L.ts_raft_corr_pyramid_fwd(one, one, one, 1, 4, 2, 1, 1, None) == -2 and b"W >= 2" in L.ts_last_error_string()
    assert L.ts_raft_corr_pyramid_fwd(one, one, one, 1, 4, 2, 16, 0, None) == -2 and b"num_levels" in L.ts_last_error_string()
    assert L.ts_raft_corr_pyramid_fwd(one, one, one, 1, 4, 2, 1024, 8, None) == -3
    assert L.ts_raft_corr_pyramid_fwd(one, None, one, 1, 4, 2, 16, 2, None) == -1 and b"NULL" in L.ts_last_error_string()
    assert L.ts_raft_corr_lookup_fwd(one, one, one, 1, 2, 16, 2, -1, None) == -2 and b"radius" in L.ts_last_error_string()
    assert L.ts_raft_corr_lookup_bwd(one, one, one, None, None, 1, 2, 16, 2, 1, 1, None) == -1
    assert L.ts_raft_corr_lookup_bwd(None, one, one, one, None, 1, 2, 16, 2, 1, 1, None) == -1        # grad_disp needs the pyramid
    assert L.ts_raft_corr_pyramid_bwd(one, one, one, None, None, 1, 4, 2, 16, 1, None) == -1
    assert L.ts_version() >= 15
