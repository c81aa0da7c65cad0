"""CPU: the host logic of the split-input entries (include/ts_hip.h) -- which seams the *_split_supported queries accept, and that
the entries refuse the others before anything is launched (no GPU here; the kernels are held to bit equality in
tests/test_split_input_gpu.py)."""
import pytest


@pytest.fixture(scope="module")
def L():
    from temporalstereo_amd import build, _lib
    build.build(verbose=False)
    return _lib.lib()


def test_supported_queries(L):
    for cs, ok in ((32, 1), (64, 1), (96, 1), (0, 0), (128, 0), (20, 0), (16, 0), (-32, 0), (160, 0)):
        assert L.ts_block_cost_corr_split_supported(128, cs) == ok, cs
        assert L.ts_conv3d_d_split_supported(128, cs) == ok, cs
        assert L.ts_conv3d_hw_x6_split_supported(128, cs, 32, 240, 1) == ok, cs
        assert L.ts_conv3d_hw_split_supported(1, 128, cs, 8, 1, 136, 240, 1, 1, 0) == ok, cs
    assert L.ts_block_cost_corr_split_supported(36, 32) == 0                       # C % 8 != 0
    assert L.ts_conv3d_hw_x6_split_supported(128, 64, 8, 240, 1) == 0              # Cout <= 8 is not an x6 layer
    assert L.ts_conv3d_hw_x6_split_supported(128, 64, 32, 38, 1) == 0              # W % 4 != 0
    assert L.ts_conv3d_hw_split_supported(1, 128, 64, 8, 1, 136, 240, 2, 1, 1) == 0          # transposed
    # a split-K launch cuts the channels into slices that start chunk sequences of their own: whole 32-channel chunks only
    assert L.ts_conv3d_hw_split_supported(1, 64, 32, 8, 1, 9, 37, 1, 1, 0) == 1               # two slices of 32
    assert L.ts_conv3d_hw_split_supported(1, 160, 64, 8, 1, 9, 37, 1, 1, 0) == 0              # two slices of 80
    assert L.ts_conv3d_hw_split_supported(1, 160, 64, 8, 1, 544, 960, 1, 1, 0) == 1           # 2,040 tiles: two workgroups per CU already, no slices


@pytest.mark.parametrize("cs", [20, 0, 64])
def test_entries_refuse_a_bad_seam_before_any_launch(L, cs):
    p, plane = 4096, 8 * 40            # any non-NULL address: a refused call never dereferences or launches
    rcs = [
        L.ts_conv3d_hw_split_fwd(p, p, p, p, p, p, 1, 64, cs, 32, 1, 8, 40, 1, 1, 0, 0, 0.0, 64 * plane, plane, 64 * plane, plane,
                                 32 * plane, plane, None, 0, None, 0, None),
        L.ts_conv3d_d_split_fwd(p, p, p, p, p, p, 1, 64, cs, 32, 1, 8, 40, 1, 1, 1, 0, 0, 0, 0.0, 64 * plane, plane, 64 * plane, plane,
                                32 * plane, plane, None),
        L.ts_conv3d_hw_x6_split_fwd(p, p, p, p, p, p, 1, 64, cs, 32, 1, 8, 40, 1, 0, 0.0, 64 * plane, plane, 64 * plane, plane,
                                    32 * plane, plane, None, 0, None, 0, None),
        L.ts_block_cost_sampled_corr_split_fwd(p, p, p, p, p, p, p, 1, 64, cs, 8, 40, 5, 3, 64 * plane, 64 * plane, 64 * plane,
                                               64 * plane, None),
    ]
    assert rcs == [-3] * 4, rcs
    assert b"Csplit" in L.ts_last_error_string()


def test_second_base_may_not_be_null(L):
    p, plane = 4096, 8 * 40
    rc = L.ts_conv3d_d_split_fwd(p, None, p, p, p, p, 1, 64, 32, 32, 1, 8, 40, 1, 1, 1, 0, 0, 0, 0.0, 64 * plane, plane, 32 * plane,
                                 plane, 32 * plane, plane, None)
    assert rc == -1 and b"NULL" in L.ts_last_error_string()
