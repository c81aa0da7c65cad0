"""CPU: the 2-D inverse warp without a GPU -- tests/warp_ref.py (the torch restatement the GPU tests take their fp64 expectations and
gradients from) is pinned to the reference's own runs in tests/golden/inverse_warp_*.npz; the argument checks of
ts_inverse_warp_fwd / ts_inverse_warp_bwd, which come before any launch; the errors the wrapper raises itself."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

import warp_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "inverse_warp_*.npz")))
MODES = ("disparity", "flow", "depth")
PADS = ("zeros", "border", "reflection")


def test_the_fixtures_are_there():
    assert FIXTURES == ["inverse_warp_a", "inverse_warp_b", "inverse_warp_c", "inverse_warp_e"]


@pytest.mark.parametrize("name", FIXTURES)
def test_warp_ref_reproduces_the_reference(name):
    g = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    t = lambda k: torch.from_numpy(g[k])
    for mode in MODES:
        geo = (t("K"), t("inv_K"), t("T")) if mode == "depth" else (None, None, None)
        for pad in PADS:
            out, side = R.inverse_warp(t("img"), t("motion_" + mode), mode, *geo, "bilinear", pad)
            key = "%s_%s" % (mode, pad)
            assert out.dtype == torch.float32 and out.shape == t("out_" + key).shape
            assert float((out - t("out_" + key)).abs().max()) <= float(g["dev_" + key]), key
        if mode == "depth":
            assert sorted(side) == sorted(k[5:] for k in g if k.startswith("side_"))
            assert torch.equal(side["flow_mask"], t("side_flow_mask"))
            assert 0.2 < float(side["flow_mask"].float().mean()) < 0.9              # the mask is neither empty nor full
            for k in ("triangular_depth", "src_pixel_coord", "optical_flow", "homo_points_3d"):
                assert side[k].shape == t("side_" + k).shape
                assert float((side[k] - t("side_" + k)).abs().max()) <= float(g["dev_side_" + k]), k
        else:
            assert side == {}


@pytest.fixture(scope="module")
def L():
    from temporalstereo_amd import _lib
    return _lib.lib()


P = 0x1000          # a non-NULL pointer that is never dereferenced: every call below is refused before any launch


def fwd(L, img=P, motion=P, K=None, inv_K=None, T=None, out=P, sizes=(1, 3, 8, 8, 8, 8), mode=0, interp=0, pad=0, kd=0, ikd=0):
    return L.ts_inverse_warp_fwd(img, motion, K, inv_K, T, out, None, None, None, None, None, *sizes, mode, interp, pad, kd, ikd, 1e-7, None)


def bwd(L, img=P, motion=P, K=None, inv_K=None, T=None, gout=P, gimg=P, gmotion=P, sizes=(1, 3, 8, 8, 8, 8), mode=0, interp=0, pad=0,
        kd=0, ikd=0):
    return L.ts_inverse_warp_bwd(img, motion, K, inv_K, T, gout, gimg, gmotion, *sizes, mode, interp, pad, kd, ikd, 1e-7, None)


def test_abi_refusals_without_gpu(L):
    assert L.ts_version() >= 14
    # NULL required pointers
    for kw in (dict(img=None), dict(motion=None), dict(out=None)):
        assert fwd(L, **kw) == -1 and b"NULL" in L.ts_last_error_string()
    for kw in (dict(motion=None), dict(gout=None), dict(gimg=None, gmotion=None), dict(img=None)):
        assert bwd(L, **kw) == -1
    # the reference divides by H - 1 and W - 1; grid_sample's un-normalisation degenerates at Hi, Wi = 1
    for sizes in ((1, 3, 8, 8, 8, 1), (1, 3, 1, 8, 8, 8), (1, 3, 8, 8, 1, 8), (1, 3, 8, 1, 8, 8), (0, 3, 8, 8, 8, 8), (1, 0, 8, 8, 8, 8),
                  (1, 3, 8, 8, 8, -4)):
        assert fwd(L, sizes=sizes) == -2 and bwd(L, sizes=sizes) == -2, sizes
    assert fwd(L, None, None, out=None, sizes=(1, 3, 8, 8, 8, 1)) == -2                # sizes come before pointers
    # codes
    assert fwd(L, interp=2) == -3 and b"bicubic" in L.ts_last_error_string()
    assert bwd(L, interp=2) == -3
    for kw in (dict(mode=3), dict(mode=-1), dict(interp=7), dict(pad=3), dict(pad=-1)):
        assert fwd(L, **kw) == -3 and bwd(L, **kw) == -3, kw
    # depth mode needs K, inv_K and T
    assert fwd(L, mode=2, K=None, inv_K=P, T=P, kd=3, ikd=3) == -1 and b"K" in L.ts_last_error_string()
    assert fwd(L, mode=2, K=P, inv_K=P, T=None, kd=3, ikd=3) == -1 and b"T_target_to_source" in L.ts_last_error_string()
    assert fwd(L, mode=2, K=P, inv_K=None, T=P, kd=3, ikd=3) == -1
    assert bwd(L, mode=2, K=None, inv_K=P, T=P, kd=3, ikd=3) == -1
    assert fwd(L, mode=2, K=P, inv_K=P, T=P, kd=5, ikd=3) == -2


def test_both_entries_can_be_recorded(L):
    from temporalstereo_amd import _lib
    w = (ctypes.c_ulonglong * 32)()
    plan = L.ts_plan_create()
    for n in ("ts_inverse_warp_fwd", "ts_inverse_warp_bwd"):
        assert n not in _lib._QUERIES
        assert L.ts_plan_add_call(plan, n.encode(), w, len(_lib.SIGNATURES[n][1])) == 0
    assert L.ts_plan_run(plan) == -2                                                   # empty arguments: refused, not launched
    L.ts_plan_destroy(plan)


def test_wrapper_errors():
    import temporalstereo_amd as ts
    img, disp = torch.zeros(1, 3, 4, 5), torch.zeros(1, 1, 4, 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ts.inverse_warp(img, disp)
    with pytest.raises(TypeError, match=r"Inverse warp only support \[disparity, flow, depth\] mode, but affine got"):
        ts.inverse_warp(img, disp, mode='affine')
    with pytest.raises(AssertionError, match="Disparity map must be 1 channel, but 2 got!"):
        ts.inverse_warp(img, torch.zeros(1, 2, 4, 5))
    with pytest.raises(AssertionError, match="Optical flow map must be 2 channel, but 1 got!"):
        ts.inverse_warp(img, disp, mode='flow')
    K, T = torch.eye(3)[None], torch.eye(4)[None]
    with pytest.raises(ValueError, match="T_target_to_source"):
        ts.inverse_warp(img, disp, mode='depth', K=K)
    with pytest.raises(RuntimeError, match="requires grad"):
        ts.inverse_warp(img, disp, mode='depth', K=K.clone().requires_grad_(True), T_target_to_source=T)
    with pytest.raises(RuntimeError, match="requires grad"):
        ts.inverse_warp(img, disp, mode='depth', K=K, T_target_to_source=T.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ts.inverse_warp(img, disp, mode='depth', K=K, T_target_to_source=T)
    # K, inv_K and T are indexed by the motion's batch element: wrong batch sizes and shapes are refused, not read past
    img2, disp2 = torch.zeros(2, 3, 4, 5), torch.zeros(2, 1, 4, 5)
    for kw in (dict(K=K, T_target_to_source=T.repeat(2, 1, 1)), dict(K=K.repeat(2, 1, 1), T_target_to_source=T),
               dict(K=K.repeat(2, 1, 1), inv_K=K, T_target_to_source=T.repeat(2, 1, 1)),
               dict(K=torch.eye(3).repeat(2, 1, 1)[:, :2], T_target_to_source=T.repeat(2, 1, 1)),
               dict(K=torch.eye(5).repeat(2, 1, 1), T_target_to_source=T.repeat(2, 1, 1)),
               dict(K=K.repeat(2, 1, 1), T_target_to_source=torch.eye(3).repeat(2, 1, 1))):
        with pytest.raises(ValueError, match="must be"):
            ts.inverse_warp(img2, disp2, mode='depth', **kw)


def test_mesh_grid_is_the_pixel_grid():
    import temporalstereo_amd as ts
    g = ts.mesh_grid(2, 3, 4, torch.device("cpu"), torch.float64)
    assert g.shape == (2, 2, 3, 4) and g.dtype == torch.float64
    assert torch.equal(g[1, 0], torch.arange(4.0, dtype=torch.float64).expand(3, 4))
    assert torch.equal(g[0, 1], torch.arange(3.0, dtype=torch.float64).view(3, 1).expand(3, 4))
    xs, ys = R.pixel_grid(2, 3, 4, g)
    assert torch.equal(g[:, 0], xs) and torch.equal(g[:, 1], ys)
