"""SPP3D without a GPU: tests/spp3d_ref.py (the plain-torch restatement, the fp64 yardstick of tests/test_spp3d_gpu.py) and
temporalstereo_amd.SPP3D on CPU tensors against the reference's own runs in tests/golden/spp3d_*.npz (tools/gen_golden.py --only-spp3d);
the state-dict contract; the argument checks of the new C-ABI entries (they come before any launch).

Bars: the fixture's recorded deviation of the reference's fp32 run from its fp64 run.  spp3d_ref in fp64 stands where the reference's
fp64 run stands, so it lies within dev_* (+ 1e-9) of the stored fp32 values; an fp32 evaluation (spp3d_ref's, or the module's CPU path,
which is the reference's op sequence) is a second fp32 run: within 4 x dev_* of the stored one (twice would be the triangle inequality if
both had the same deviation; the factor 4 as in tests/test_raft_corr_gpu.py).  Gradients: relative L2 <= 4 x rel_grad_* + 1e-6.
"""
import pytest
import torch

import spp3d_ref as R
from compare import T, err, rel_l2
import temporalstereo_amd as ts
from temporalstereo_amd import _lib

FIXTURES = ("a", "b", "c", "d")
STRIDES = (2, 4, 8, 16)


@pytest.mark.parametrize("tag", FIXTURES)
def test_ref_reproduces_the_fixture(tag):
    g = R.load_fixture(tag)
    B, C, D, H, W = g["shape"]
    assert g["strides"] == STRIDES
    for dt, k in ((torch.float64, 1.0), (torch.float32, 4.0)):
        with torch.no_grad():
            run = R.spp3d(R.fixture_input(g["seed"], g["shape"], dt), R.fixture_state(g["seed"], C, 4, dt), STRIDES, g["training"])
        assert err(run["out"], T(g["out"])) <= k * float(g["dev_out"]) + 1e-9
        assert err(R.sample(run["cat"][:, C:], g["cat_idx"]), T(g["cat_val"])) <= k * float(g["dev_cat"]) + 1e-9
        assert torch.equal(run["cat"][:, :C], R.fixture_input(g["seed"], g["shape"], dt))
        for i, p in enumerate(run["pooled"]):
            assert err(p, T(g["pooled_%d" % i])) <= k * float(g["dev_pooled_%d" % i]) + 1e-9
        for key, v in run["stats"].items():
            if key.endswith("num_batches_tracked"):
                assert int(v) == int(g["stat_" + key]) == 1
            else:
                assert err(v, T(g["stat_" + key])) <= k * float(g["dev_stat_" + key]) + 1e-9


@pytest.mark.parametrize("tag", ("a", "b", "c"))
def test_ref_gradients_reproduce_the_fixture(tag):
    g = R.load_fixture(tag)
    C = g["shape"][1]
    state = {k: (v.requires_grad_("running" not in k) if v.is_floating_point() else v)
             for k, v in R.fixture_state(g["seed"], C, 4, torch.float64).items()}
    x = R.fixture_input(g["seed"], g["shape"], torch.float64).requires_grad_(True)
    out = R.spp3d(x, state, STRIDES, True)["out"]
    out.backward(R.fixture_cotangent(g["seed"], out.shape, torch.float64))
    assert rel_l2(T(g["grad_x"]), x.grad) <= float(g["rel_grad_x"]) * (1 + 1e-6) + 1e-9
    for k, v in state.items():
        if v.is_floating_point() and v.grad is not None:
            assert rel_l2(T(g["grad_" + k]), v.grad) <= float(g["rel_grad_" + k]) * (1 + 1e-6) + 1e-9, k


@pytest.mark.parametrize("tag", FIXTURES)
def test_module_on_cpu_tensors_equals_the_fixture(tag):
    g = R.load_fixture(tag)
    B, C, D, H, W = g["shape"]
    m = ts.SPP3D(in_planes=C, strides=STRIDES)
    assert list(m.state_dict().keys()) == [str(k) for k in g["keys"]]
    m.load_state_dict(R.fixture_state(g["seed"], C, 4), strict=True)           # reference-keyed: strict-clean
    m.train(g["training"])
    x = R.fixture_input(g["seed"], g["shape"]).requires_grad_(g["training"])
    out = m(x)
    assert err(out.detach(), T(g["out"])) <= 4 * float(g["dev_out"])
    if not g["training"]:
        return
    out.backward(R.fixture_cotangent(g["seed"], out.shape))
    assert rel_l2(x.grad, T(g["grad_x"])) <= 4 * float(g["rel_grad_x"]) + 1e-6
    for k, p in m.named_parameters():
        assert rel_l2(p.grad, T(g["grad_" + k])) <= 4 * float(g["rel_grad_" + k]) + 1e-6, k
    for k, v in m.state_dict().items():
        if "running_" in k:
            assert err(v, T(g["stat_" + k])) <= 4 * float(g["dev_stat_" + k]) + 1e-9, k
        elif k.endswith("num_batches_tracked"):
            assert int(v) == 1


@pytest.mark.parametrize("shape", ((1, 8, 2, 4, 70), (1, 64, 4, 8, 12)))
def test_module_on_cpu_tensors_against_the_ref_in_fp64(shape):
    """the shapes without a fixture, eval mode ((1,64,4,8,12) has one-cell levels and B = 1: train mode refuses it, below)"""
    C = shape[1]
    state = R.fixture_state(77, C, 4)
    x = R.fixture_input(77, shape)
    m = ts.SPP3D(in_planes=C, strides=STRIDES)
    m.load_state_dict(state, strict=True)
    m.eval()
    with torch.no_grad():
        got = m(x)
        s64 = {k: (v.double() if v.is_floating_point() else v) for k, v in state.items()}
        want = R.spp3d(x.double(), s64, STRIDES, False)["out"]
        own = R.spp3d(x, state, STRIDES, False)["out"]
    assert err(got, want) <= max(4 * err(own, want), 16 * 2.0 ** -24 * float(want.abs().max()))


def test_train_mode_refuses_one_value_per_channel():
    m = ts.SPP3D(in_planes=8)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        m.train()(torch.zeros(1, 8, 1, 2, 2))
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        R.spp3d(torch.zeros(1, 8, 1, 2, 2), R.fixture_state(1, 8, 4), STRIDES, True)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        ts.SPP3D(in_planes=64).train()(torch.zeros(1, 64, 4, 8, 12))


def test_constructor_contract():
    m = ts.SPP3D()
    assert (m.in_planes, tuple(m.strides), m.norm, m.activation) == (64, (2, 4, 8, 16), 'BN3d', 'ReLU')
    assert tuple(m.fuse[0].weight.shape) == (64, 128, 3, 3, 3) and tuple(m.fuse[1].weight.shape) == (64, 64, 1, 1, 1)
    assert m.fuse[1].bias is None and m.pools[0].bias is None
    with pytest.raises(ValueError):
        ts.SPP3D(fuse_conv="other")
    assert ts.spp3d_level_sizes((5, 6, 7), STRIDES) == [(2, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1)] == R.level_sizes((5, 6, 7), STRIDES)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ts.spp3d_pool(torch.zeros(1, 2, 4, 4, 4), STRIDES)


def test_abi_version_and_argument_checks():
    """Validation happens before any launch, so it is checkable without a GPU."""
    L = _lib.lib()
    assert L.ts_version() >= 18
    one = 4096                  # any non-NULL value: the checks that are expected to fail come before a pointer is used
    # ts_spp3d_pool_fwd(x, pooled, B, C, D, H, W, L, s0..s3, x_bs, x_cs, stream)
    assert L.ts_spp3d_pool_fwd(None, one, 1, 8, 5, 6, 7, 4, 2, 4, 8, 16, 8 * 210, 210, None) == -1 and b"NULL" in L.ts_last_error_string()
    assert L.ts_spp3d_pool_fwd(one, None, 1, 8, 5, 6, 7, 4, 2, 4, 8, 16, 8 * 210, 210, None) == -1
    assert L.ts_spp3d_pool_fwd(one, one, 1, 8, 0, 6, 7, 4, 2, 4, 8, 16, 8 * 210, 210, None) == -2
    assert L.ts_spp3d_pool_fwd(one, one, 1, 8, 5, 6, 7, 0, 2, 4, 8, 16, 8 * 210, 210, None) == -2           # no level
    assert L.ts_spp3d_pool_fwd(one, one, 1, 8, 5, 6, 7, 4, 2, 0, 8, 16, 8 * 210, 210, None) == -2           # a stride of 0
    assert L.ts_spp3d_pool_fwd(one, one, 2, 8, 5, 6, 7, 4, 2, 4, 8, 16, 8 * 210, 209, None) == -2           # channels overlap
    assert L.ts_spp3d_pool_fwd(one, one, 1, 8, 5, 6, 7, 5, 2, 4, 8, 16, 8 * 210, 210, None) == -3           # five levels
    assert L.ts_spp3d_pool_fwd(one, one, 1, 8, 5, 6, 1 << 20, 4, 2, 4, 8, 16, 1 << 40, 1 << 30, None) == -3
    # ts_spp3d_pool_bwd(g0..g3, addend, grad_x, B, C, D, H, W, L, s0..s3, add_bs, add_cs, gx_bs, gx_cs, stream)
    assert L.ts_spp3d_pool_bwd(one, one, one, one, None, None, 1, 8, 5, 6, 7, 4, 2, 4, 8, 16, 0, 0, 8 * 210, 210, None) == -1
    assert L.ts_spp3d_pool_bwd(one, one, None, one, None, one, 1, 8, 5, 6, 7, 4, 2, 4, 8, 16, 0, 0, 8 * 210, 210, None) == -1
    assert L.ts_spp3d_pool_bwd(one, one, one, one, one, one, 1, 8, 5, 6, 7, 4, 2, 4, 8, 16, 0, 0, 8 * 210, 210, None) == -2    # addend strides
    assert L.ts_spp3d_pool_bwd(one, one, one, one, None, one, 1, 8, 5, 6, 7, 4, 2, 4, 8, 16, 0, 0, 8 * 210, 100, None) == -2
    # ts_spp3d_expand_fwd(x, lv0..lv3, cat, B, C, Cl, D, H, W, L, s0..s3, x_bs, x_cs, stream)
    assert L.ts_spp3d_expand_fwd(one, one, one, one, None, one, 1, 8, 16, 5, 6, 7, 4, 2, 4, 8, 16, 8 * 210, 210, None) == -1
    assert L.ts_spp3d_expand_fwd(None, one, one, one, one, one, 1, 8, 16, 5, 6, 7, 4, 2, 4, 8, 16, 8 * 210, 210, None) == -1
    assert L.ts_spp3d_expand_fwd(one, one, one, one, one, one, 1, 8, 0, 5, 6, 7, 4, 2, 4, 8, 16, 8 * 210, 210, None) == -2
    assert L.ts_spp3d_expand_fwd(one, one, one, one, one, one, 1000, 8, 16, 5, 6, 7, 4, 2, 4, 8, 16, 8 * 210, 210, None) == -3   # B * Ccat > 65535
    # ts_spp3d_expand_bwd(grad_cat, g0..g3, B, C, Cl, D, H, W, L, s0..s3, g_bs, g_cs, stream)
    assert L.ts_spp3d_expand_bwd(None, one, one, one, one, 1, 8, 16, 5, 6, 7, 4, 2, 4, 8, 16, 72 * 210, 210, None) == -1
    assert L.ts_spp3d_expand_bwd(one, one, None, one, one, 1, 8, 16, 5, 6, 7, 4, 2, 4, 8, 16, 72 * 210, 210, None) == -1
    assert L.ts_spp3d_expand_bwd(one, one, one, one, one, 1, 8, 16, 5, 6, 7, 4, 2, 4, 8, 16, 72 * 210, 209, None) == -2
    assert L.ts_spp3d_expand_bwd(one, one, one, one, one, 1, 8, 16, 5, -6, 7, 4, 2, 4, 8, 16, 72 * 210, 210, None) == -2
    # ts_depth_sum3_fwd(z0, z1, z2, scale, shift, y, B, C, D, H, W, act, 8 strides, stream)
    st = (8 * 210, 210) * 4
    assert L.ts_depth_sum3_fwd(one, one, None, None, None, one, 1, 8, 5, 6, 7, 0, *st, None) == -1
    assert L.ts_depth_sum3_fwd(one, one, one, None, None, None, 1, 8, 5, 6, 7, 0, *st, None) == -1
    assert L.ts_depth_sum3_fwd(one, one, one, None, None, one, 1, 8, 5, 6, 7, 3, *st, None) == -2              # unknown activation
    assert L.ts_depth_sum3_fwd(one, one, one, None, None, one, 1, 8, 5, 6, 0, 0, *st, None) == -2
    assert L.ts_depth_sum3_fwd(one, one, one, None, None, one, 1, 8, 5, 6, 7, 0, *((8 * 210, 100) * 4), None) == -2
    assert L.ts_depth_sum3_fwd(one, one, one, None, None, one, 1, 8, 70000, 6, 7, 0, *((8 * 70000 * 42, 70000 * 42) * 4), None) == -3
    # ts_bn_small_train_bwd(y, g, gamma, beta, sum_g, sum_gx, dy, B, C, N, 6 strides, eps, act, stream)
    st6 = (16 * 3, 3) * 3
    assert L.ts_bn_small_train_bwd(one, one, None, None, one, one, None, 2, 16, 3, *st6, 1e-5, 2, None) == -1
    assert L.ts_bn_small_train_bwd(None, one, None, None, one, one, one, 2, 16, 3, *st6, 1e-5, 2, None) == -1
    assert L.ts_bn_small_train_bwd(one, one, None, None, one, one, one, 1, 16, 1, *((16, 1) * 3), 1e-5, 2, None) == -2      # one value per channel
    assert L.ts_bn_small_train_bwd(one, one, None, None, one, one, one, 2, 16, 3, *((16 * 3, 2) * 3), 1e-5, 2, None) == -2
    assert L.ts_bn_small_train_bwd(one, one, None, None, one, one, one, 2, 16, 3, *st6, 1e-5, 5, None) == -2
    assert L.ts_bn_small_train_bwd(one, one, None, None, one, one, one, 2, 16, 4096, *((16 * 4096, 4096) * 3), 1e-5, 2, None) == -3


def test_frozen_batchnorms_run_where_train_mode_refuses():
    """the refusal follows each BatchNorm's own mode, as F.batch_norm's does: a module in train() whose BatchNorms are in eval() runs a
    one-cell level with B = 1 (running statistics), on the module's own path and on the reference's op sequence alike"""
    m = ts.SPP3D(in_planes=8).train()
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm3d):
            mod.eval()
    x = R.fixture_input(3, (1, 8, 1, 2, 2))
    assert torch.equal(m(x), m._reference_forward(x))


def test_fixture_sizes():
    """what the fixtures hold fixes their sizes (PROVENANCE_spp3d.txt): out and grad_x of shape b are 343 KB each, the weight gradient
    of fuse.0 of shape c 331 KB; nothing else may grow them, and no file comes near the 1 MiB a committed file may have"""
    import os
    for tag, cap in (("a", 128), ("b", 800), ("c", 576), ("d", 32)):
        assert os.path.getsize(os.path.join(R.GOLDEN, "spp3d_%s.npz" % tag)) <= cap * 1024, tag
