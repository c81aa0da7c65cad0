"""GPU: the fused regression tails of an inference pass (ts_regress_convex_upsample_fwd, ts_topk_softargmax_half_fwd,
ts_deconv2d_k4s2_unet_upsample_fwd) against the two launches each replaces, on the same seeded inputs.  Every comparison is
torch.equal: the fused kernels share the per-pixel arithmetic of the stand-alone ones (csrc/regress_tails.hpp), so a difference in the
last bit is a bug."""
import pytest
import torch

import synth
from helpers import t

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _rand(seed, *shape, scale=1.0, dev=None):
    return t(synth.normal(seed, "x%d" % len(shape), shape, scale), dev)


def _st():
    from temporalstereo_amd import _lib
    return _lib.ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------- entry 1
def _topk(cost, samp, off, k):
    from temporalstereo_amd import _lib
    B, D, H, W = cost.shape
    disp = torch.empty((B, 1, H, W), device=cost.device)
    td, tc = torch.empty((B, k, H, W), device=cost.device), torch.empty((B, k, H, W), device=cost.device)
    _lib.check(_lib.lib().ts_topk_softargmax_fwd(_lib.ptr(cost), _lib.ptr(samp), _lib.ptr(off), _lib.ptr(disp), _lib.ptr(td),
                                                 _lib.ptr(tc), None, B, D, H, W, k, _st()), "ts_topk_softargmax_fwd")
    return disp, td, tc


def _convex_pair(cost, samp, off, mask, k, r, rng, front):
    """(out, low, high, candidates) of today's two launches and of the fused one; unwritten leading planes stay zero in both."""
    from temporalstereo_amd import _lib
    B, D, H, W = cost.shape
    mk = lambda c: torch.zeros((B, c, H * r, W * r), device=cost.device)
    disp, _, _ = _topk(cost, samp, off, k)
    want = [mk(1), mk(1), mk(1), mk(front + 5)]
    _lib.check(_lib.lib().ts_convex_upsample_candidates_fwd(_lib.ptr(mask), _lib.ptr(disp), *[_lib.ptr(x) for x in want], B, H, W, r,
                                                            float(r), rng, front, front + 5, _st()), "ts_convex_upsample_candidates_fwd")
    got = [mk(1), mk(1), mk(1), mk(front + 5)]
    _lib.check(_lib.lib().ts_regress_convex_upsample_fwd(_lib.ptr(cost), _lib.ptr(samp), _lib.ptr(off), _lib.ptr(mask),
                                                         *[_lib.ptr(x) for x in got], B, D, H, W, k, r, float(r), rng, front, front + 5,
                                                         _st()), "ts_regress_convex_upsample_fwd")
    torch.cuda.synchronize()
    return want, got


def _level_inputs(seed, B, D, H, W, r, dev, logit_scale=1.0):
    cost = _rand(seed, B, D, H, W, dev=dev)
    samp = t(synth.uniform(seed + 1, "s", (B, D, H, W), 0.0, 40.0), dev)
    off = _rand(seed + 2, B, D, H, W, scale=0.3, dev=dev)
    mask = _rand(seed + 3, B, 9 * r * r, H, W, scale=logit_scale, dev=dev)
    return cost, samp, off, mask


@pytest.mark.parametrize("front", [0, 2])
@pytest.mark.parametrize("hw", [(5, 7), (9, 19)])          # smaller than an 8x8 block; ragged in both axes, 2 x 3 blocks
@pytest.mark.parametrize("D", [7, 14])                     # the 8-wide load blocks: exact + ragged, and ragged alone
def test_regress_convex_upsample_equals_the_two_launches(D, hw, front):
    dev = _dev()
    cost, samp, off, mask = _level_inputs(100 + D, 2, D, hw[0], hw[1], 2, dev)
    want, got = _convex_pair(cost, samp, off, mask, 2, 2, 4.0, front)
    for a, b, what in zip(got, want, ("out", "low", "high", "candidates")):
        assert torch.equal(a, b), what


def test_regress_convex_upsample_ties_keep_the_lowest_index():
    """Whole columns of equal costs: the top-k of such a pixel is candidates 0 and 1 in that order, in both forms."""
    dev = _dev()
    cost, samp, off, mask = _level_inputs(131, 2, 7, 9, 19, 2, dev)
    cost[:, :, :, 3] = 0.25
    cost[:, :, :, 8:11] = -1.5
    cost[:, :, :, 18] = 0.0
    want, got = _convex_pair(cost, samp, off, mask, 2, 2, 4.0, 0)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    _, td, _ = _topk(cost, samp, off, 2)
    assert torch.equal(td[:, :, :, 3], (samp + off)[:, :2, :, 3])


def test_regress_convex_upsample_wide_logits():
    dev = _dev()
    cost, samp, off, mask = _level_inputs(141, 2, 14, 9, 19, 2, dev, logit_scale=30.0)
    want, got = _convex_pair(cost, samp, off, mask, 2, 2, 4.0, 0)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert bool(torch.isfinite(got[0]).all())


# ------------------------------------------------------------------------------------------- entry 2
def _half(cost, samp, off, k):
    from temporalstereo_amd import _lib
    B, D, H, W = cost.shape
    disp = torch.zeros((B, 1, H, W), device=cost.device)
    ms, mc = torch.zeros((B, k, H // 2, W // 2), device=cost.device), torch.zeros((B, k, H // 2, W // 2), device=cost.device)
    rc = _lib.lib().ts_topk_softargmax_half_fwd(_lib.ptr(cost), _lib.ptr(samp), _lib.ptr(off), _lib.ptr(disp), _lib.ptr(ms),
                                                _lib.ptr(mc), B, D, H, W, k, _st())
    return rc, disp, ms, mc


@pytest.mark.parametrize("hw", [(6, 10), (20, 36)])        # one tile; 2 x 3 tiles of 16 x 16 pixels, ragged in both axes
def test_topk_softargmax_half_equals_regression_then_resize(hw):
    from temporalstereo_amd.aggregation import native
    dev = _dev()
    cost, samp, off, _ = _level_inputs(151, 2, 5, hw[0], hw[1], 1, dev)
    disp, td, tc = _topk(cost, samp, off, 2)
    ws, wc = native.resize_bilinear_pair(td, tc, (hw[0] // 2, hw[1] // 2), 0.5, 1.0)
    rc, gd, gs, gc = _half(cost, samp, off, 2)
    torch.cuda.synchronize()
    assert rc == 0
    assert torch.equal(gd, disp) and torch.equal(gs, ws) and torch.equal(gc, wc)


def test_topk_softargmax_half_refuses_odd_sizes():
    """(The entry is not wired into NativePrecise -- it did not pay, DESIGN section 9 -- so there is no fall-back to test: the level
    always runs the regression and the resize as two launches.)"""
    from temporalstereo_amd import _lib
    dev = _dev()
    cost, samp, off, _ = _level_inputs(161, 2, 5, 7, 10, 1, dev)
    rc, gd, gs, gc = _half(cost, samp, off, 2)
    assert rc == -3 and b"odd size" in _lib.lib().ts_last_error_string()          # TS_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert not gd.any() and not gs.any() and not gc.any()                          # nothing was launched


# ------------------------------------------------------------------------------------------- entry 3
@pytest.mark.parametrize("cin,hw,wscale", [(32, (5, 10), 1.0), (24, (9, 40), 1.0), (32, (9, 40), 10.0)])
def test_deconv_unet_upsample_equals_the_two_launches(cin, hw, wscale):
    """Disparity 5 x 10: one partial tile of the deconvolution's 4 x 32 input pixels; 9 x 40: partial tiles in both axes (80 input
    columns = 2.5 tiles).  24 input channels: three 8-channel chunks."""
    from temporalstereo_amd import _lib
    dev = _dev()
    L = _lib.lib()
    B, (h, w), cout = 2, hw, 9
    H2, W2, Ho, Wo = 2 * h, 2 * w, 4 * h, 4 * w
    pad = int(L.ts_conv_cout_pad(cout))
    x = _rand(171, B, cin, H2, W2, dev=dev)
    w_t = _rand(172, cin, 16, pad, scale=wscale / (4.0 * cin ** 0.5), dev=dev)
    scale = t(synth.uniform(173, "sc", (pad,), 0.5, 1.5), dev)
    shift = _rand(174, pad, scale=0.2, dev=dev)
    disp = t(synth.uniform(175, "d", (B, 1, h, w), 0.0, 40.0), dev)
    w6 = torch.empty(int(L.ts_conv3d_hw_x6s_weight_bytes(cin, cout, 2)), device=dev, dtype=torch.uint8)
    _lib.check(L.ts_conv3d_hw_x6s_weight_split(_lib.ptr(w_t), _lib.ptr(w6), cin, cout, pad, 2, _st()), "ts_conv3d_hw_x6s_weight_split")
    mask = torch.empty((B, cout, Ho, Wo), device=dev)
    _lib.check(L.ts_conv3d_hw_x6s_fwd(_lib.ptr(x), _lib.ptr(w6), _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(mask), B, cin, cout, 1, H2, W2,
                                      2, 0, 0.0, cin * H2 * W2, H2 * W2, cout * Ho * Wo, Ho * Wo, _st()), "ts_conv3d_hw_x6s_fwd")
    want = torch.zeros((B, 1, Ho, Wo), device=dev)
    _lib.check(L.ts_unet_upsample_fwd(_lib.ptr(mask), _lib.ptr(disp), _lib.ptr(want), B, h, w, Ho, Wo, _st()), "ts_unet_upsample_fwd")
    got = torch.zeros((B, 1, Ho, Wo), device=dev)
    _lib.check(L.ts_deconv2d_k4s2_unet_upsample_fwd(_lib.ptr(x), _lib.ptr(w6), _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(disp),
                                                    _lib.ptr(got), B, cin, cout, H2, W2, cin * H2 * W2, H2 * W2, _st()),
               "ts_deconv2d_k4s2_unet_upsample_fwd")
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert float(want.abs().max()) > 1.0


# ------------------------------------------------------------------------------------------- the whole pass
def test_pipelined_plan_is_three_launches_shorter_and_bit_identical(monkeypatch):
    """The pipelined batch-1 pass at the smallest geometry of tests/test_native_gpu.py, recorded with the fused tails on and off: equal
    outputs, and the recorded plan loses the coarse and fine levels' regressions and the UNet upsampling.  Three launches, not the
    four of the design: the fourth (the 1/4 level's regression with the memory resize, ts_topk_softargmax_half_fwd) measured within
    noise of the two launches it replaces and is not wired in, so that level still records both.  (At this size the last
    deconvolution's grid is below the x6s kernel's threshold, where the pass keeps the two launches by design: the threshold is
    lowered for both arms so that the fused deconvolution is what is recorded.)"""
    import bench
    import temporalstereo_amd as ts
    from temporalstereo_amd.aggregation import native
    from temporalstereo_amd.aggregation.engine import InferenceEngine
    dev = _dev()
    seed = synth.SEED0 + 7
    net = ts.TEMPORALSTEREO(coarse=ts.CoarseAggregation(32, 8, 4), fine=ts.FineAggregation(16, 8, 5), precise=ts.PreciseAggregation(8, 8, 5))
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.state_values(shapes, seed).items()}, strict=True)
    net = net.to(dev)
    B, H, W = 1, 96, 160
    lf, rf = synth.feature_pyramid(seed, B, H, W, chans=(8, 16, 32))
    il, ir = synth.images(seed, B, H, W)
    frame = ([torch.from_numpy(x).to(dev) for x in lf], [torch.from_numpy(x).to(dev) for x in rf],
             torch.from_numpy(il).to(dev), torch.from_numpy(ir).to(dev))
    bench.calibrate_batchnorm(net, frame)
    monkeypatch.setattr(native, "_X6S_MIN_GRID", 1)
    outs, logs = {}, {}
    for fused in (False, True):
        monkeypatch.setattr(native, "FUSED_TAILS", native._fused_tails("1" if fused else "0"))
        eng = InferenceEngine(net, backend="native", replay="plan", inputs="bind", pipeline=2)
        res = [eng(*frame, {}) for _ in range(3)]                    # two recordings, then a replay of the first
        torch.cuda.synchronize()
        outs[fused] = [[x.clone() for x in r[0]] for r in res]
        logs[fused] = [[name for name, _ in cap.recorder.log] for cap in eng._graphs.values()]
    assert all(torch.equal(a, b) for ra, rb in zip(outs[True], outs[False]) for a, b in zip(ra, rb))
    count = lambda log, name: sum(n == name for n in log)
    for on, off in zip(logs[True], logs[False]):
        assert len(off) - len(on) == 3
        assert count(off, "ts_topk_softargmax_fwd") == 3 and count(on, "ts_topk_softargmax_fwd") == 1
        assert count(off, "ts_unet_upsample_fwd") == 1 and count(on, "ts_unet_upsample_fwd") == 0
        assert count(off, "ts_resize_bilinear_pair_fwd") == count(on, "ts_resize_bilinear_pair_fwd")
        assert count(on, "ts_regress_convex_upsample_fwd") == 2 and count(on, "ts_deconv2d_k4s2_unet_upsample_fwd") == 1
