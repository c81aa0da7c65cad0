"""SPP3D on the device (temporalstereo_amd.SPP3D / spp3d_pool / spp3d_expand / conv3d_k333; csrc/spp3d.hip) against the reference's own
runs recorded in tests/golden/spp3d_*.npz (tools/gen_golden.py --only-spp3d) and against tests/spp3d_ref.py and the framework's
operators in fp64 on the CPU.  u = 2^-24.

Bars, none taken from the code under test:
  pool        |hip - fp64| <= (n + 2) u (mean |x| over the box), n the box volume: an fp32 sum of n terms in any order, and the division.
              Backward against fp64 autograd: (L + 3) u sum_i |g_i| / |k_i| (L + 1 terms in the same form); bit-equal over two runs.
  expand      channels [0, C) bit-equal to x; a one-cell level bit-equal to that cell everywhere; otherwise |hip - fp64 interpolate| <=
              max(4 x the deviation of the framework's own fp32 F.interpolate from its fp64 on the same input, 16 u max |level|).
              Backward against fp64 autograd, at the same ratio: max(4 x the deviation of the framework's own fp32 backward from its
              fp64 on the same input, 16 u max |gradient|); bit-equal over two runs.
  conv3d_k333 forward |err| <= (27 Cin + 8) u max over outputs of sum |w||x| (fp64); gradients: relative L2 <= max(4 x fp32 CPU
              F.conv3d's own, 1e-6).
  module      output, stored stages, running statistics: |hip - fp64| <= max(4 x dev_*, the stage's floor: the pool bound, 16 u max |.|
              for the concatenation, the output and the statistics).  Gradients against fp64: max(4 x rel_grad_*, 1e-6); against the
              stored fp32 gradients: that plus rel_grad_* (triangle inequality).  The factor 4 is argued in tests/test_raft_corr_gpu.py.
Shape f, (1,64,4,8,12), has B = 1 and one cell at strides 8 and 16: train mode refuses it, in the reference too (asserted); its values and
gradients are checked in eval mode.
A level of few cells gives its train-mode BatchNorm down to two values per channel; its output then hardly depends on its input and
the gradient that reaches the 1x1x1 weight is what is left of a cancellation, O(eps / var) of its terms.  SPP3D asks for the fp64
BatchNorm backward there (ts_bn_small_train_bwd, checked alone below); with the fp32 one this gradient sat at 3.5e-04 .. 2.3e-03 of
its norm, which is the range of the reference's own fp32 run (3.4e-05 .. 2.3e-03) and above 4 x its luckiest value.
Each case prints error / bar; with TS_SPP3D_PARITY_FILE set the line is appended to that file (profiles/spp3d_parity.txt is made so).
"""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import spp3d_ref as R
from compare import U, Parity, dev as _dev, gpu, rel_l2, same_bits
import temporalstereo_amd as ts
from temporalstereo_amd import functional as TF

pytestmark = pytest.mark.gpu

P = Parity("TS_SPP3D_PARITY_FILE", width=44)
report, check = P.report, P.check
STRIDES = (2, 4, 8, 16)
#        tag  B  C   D   H   W   training
SHAPES = {"a": (2, 8, 5, 6, 7, True),          # clamped boxes that are no multiples, dropped plane and column, one-cell levels, batch stride
          "b": (1, 8, 18, 17, 35, True),       # no clamp: a chain of nested boxes; a remainder on every axis
          "c": (2, 32, 3, 9, 20, True),        # clamp in D only; Ccat = 96
          "d": (1, 8, 1, 2, 2, False),         # every level one cell; eval
          "e": (1, 8, 2, 4, 70, False),        # a row longer than a 64-wide tile (no fixture)
          "f": (1, 64, 4, 8, 12, False)}       # the default in_planes, Ccat = 128 (no fixture).  Strides 8 and 16 leave one cell and B = 1:
#                                                  train mode refuses it (asserted below), as the reference does; values and gradients in eval mode
FIXTURES = ("a", "b", "c", "d")
TAGS = tuple(SHAPES)


@functools.lru_cache(maxsize=None)
def seed_of(tag):
    return R.load_fixture(tag)["seed"] if tag in FIXTURES else 4242 + ord(tag)


@functools.lru_cache(maxsize=None)
def case(tag):
    """Inputs, the fp64 run of spp3d_ref and (train shapes) its gradients, computed once and left unchanged."""
    B, C, D, H, W, training = SHAPES[tag]
    seed = seed_of(tag)
    x = R.fixture_input(seed, (B, C, D, H, W))
    state = R.fixture_state(seed, C, len(STRIDES))
    s64 = {k: (v.double() if v.is_floating_point() else v) for k, v in state.items()}
    with torch.no_grad():
        run = R.spp3d(x.double(), s64, STRIDES, training)
    return dict(x=x, state=state, run=run)


@functools.lru_cache(maxsize=None)
def fp64_grads(tag):
    """gradients of the seeded cotangent through spp3d_ref in fp64, in the shape's own mode"""
    B, C, D, H, W, training = SHAPES[tag]
    seed = seed_of(tag)
    s64 = {k: (v.double().requires_grad_("running" not in k) if v.is_floating_point() else v) for k, v in R.fixture_state(seed, C, len(STRIDES)).items()}
    x64 = R.fixture_input(seed, (B, C, D, H, W), torch.float64).requires_grad_(True)
    run = R.spp3d(x64, s64, STRIDES, training)
    run["out"].backward(R.fixture_cotangent(seed, run["out"].shape, torch.float64))
    g = {k: v.grad for k, v in s64.items() if v.is_floating_point() and v.grad is not None}
    g["x"] = x64.grad
    return g


def module(tag, training):
    B, C = SHAPES[tag][:2]
    m = ts.SPP3D(in_planes=C, strides=STRIDES)
    m.load_state_dict(case(tag)["state"], strict=True)
    return m.to(_dev()).train(training)


# ------------------------------------------------------------------------------------------------------------------------- pool
@pytest.mark.parametrize("tag", TAGS)
def test_pool_forward_and_backward(tag):
    B, C, D, H, W, _ = SHAPES[tag]
    x = case(tag)["x"]
    want = R.pool(x.double(), STRIDES)
    mean_abs = R.pool(x.double().abs(), STRIDES)
    boxes = R.boxes((D, H, W), STRIDES)
    xg = gpu(x).requires_grad_(True)
    levels = ts.spp3d_pool(xg, STRIDES)
    assert [tuple(l.shape[2:]) for l in levels] == R.level_sizes((D, H, W), STRIDES) == ts.spp3d_level_sizes((D, H, W), STRIDES)
    for i, (l, w, a, k) in enumerate(zip(levels, want, mean_abs, boxes)):
        n = k[0] * k[1] * k[2]
        check("pool %s level %d box %s" % (tag, i, k), l.detach(), w, (n + 2) * U * a + 1e-300)
    # a channel slice of a wider tensor (batch and channel strides): the same bits
    wide = torch.zeros((B, C + 3, D, H, W), device=_dev())
    wide[:, 2:2 + C] = xg.detach()
    for l, s in zip(levels, ts.spp3d_pool(wide[:, 2:2 + C], STRIDES)):
        assert same_bits(l.detach(), s)
    # backward: seeded cotangents k / 8
    cots = [R.fixture_cotangent(seed_of(tag) + 1 + i, l.shape) for i, l in enumerate(levels)]
    x64 = x.double().requires_grad_(True)
    sum((l * c.double()).sum() for l, c in zip(R.pool(x64, STRIDES), cots)).backward()
    a64 = x.double().requires_grad_(True)
    sum((l * c.double().abs()).sum() for l, c in zip(R.pool(a64, STRIDES), cots)).backward()          # sum_i |g_i| / |k_i|
    grads = []
    for _ in range(2):
        xg.grad = None
        sum((l * gpu(c)).sum() for l, c in zip(ts.spp3d_pool(xg, STRIDES), cots)).backward()
        grads.append(xg.grad.clone())
    assert same_bits(grads[0], grads[1])
    check("pool %s grad_x" % tag, grads[0], x64.grad, (len(STRIDES) + 3) * U * a64.grad + 1e-300)


# ----------------------------------------------------------------------------------------------------------------------- expand
@pytest.mark.parametrize("tag", TAGS)
def test_expand_forward_and_backward(tag):
    B, C, D, H, W, _ = SHAPES[tag]
    x = case(tag)["x"]
    sizes = R.level_sizes((D, H, W), STRIDES)
    rng = np.random.RandomState(seed_of(tag) % (2 ** 32))
    levels = [torch.from_numpy(rng.standard_normal((B, 16) + n).astype(np.float32)) for n in sizes]
    lg = [gpu(l).requires_grad_(True) for l in levels]
    xg = gpu(x).requires_grad_(True)
    cat = ts.spp3d_expand(lg, xg, STRIDES)
    assert tuple(cat.shape) == (B, C + 16 * len(STRIDES), D, H, W)
    assert same_bits(cat[:, :C].detach(), xg.detach())
    assert same_bits(ts.spp3d_expand([l.detach() for l in lg], xg.detach()), cat.detach())          # strides inferred from the sizes
    cot = R.fixture_cotangent(seed_of(tag) + 7, cat.shape)
    cat.backward(gpu(cot))
    first = [l.grad.clone() for l in lg]
    assert same_bits(xg.grad, gpu(cot)[:, :C])
    for l in lg:
        l.grad = None
    ts.spp3d_expand(lg, xg, STRIDES).backward(gpu(cot))
    for i, (l, n) in enumerate(zip(levels, sizes)):
        got = cat[:, C + 16 * i:C + 16 * (i + 1)].detach()
        l64, l32 = l.double().requires_grad_(True), l.clone().requires_grad_(True)
        w64 = F.interpolate(l64, size=(D, H, W), mode="trilinear", align_corners=True)
        w32 = F.interpolate(l32, size=(D, H, W), mode="trilinear", align_corners=True)
        if n == (1, 1, 1):
            assert same_bits(got, gpu(l).expand(B, 16, D, H, W)), (tag, i)
        else:
            dev = float((w32.detach().double() - w64.detach()).abs().max())
            check("expand %s level %d %s" % (tag, i, n), got, w64.detach(), max(4 * dev, 16 * U * float(l.abs().max())))
        c = cot[:, C + 16 * i:C + 16 * (i + 1)]
        w64.backward(c.double())
        w32.backward(c)
        dev = float((l32.grad.double() - l64.grad).abs().max())
        check("expand %s level %d grad" % (tag, i), first[i], l64.grad, max(4 * dev, 16 * U * float(l64.grad.abs().max())))
        assert same_bits(first[i], lg[i].grad), (tag, i)


# ------------------------------------------------------------------------------------------------------------------ conv3d_k333
@functools.lru_cache(maxsize=None)
def conv_case(cin, D):
    cout, H, W = {72: (8, 6, 7), 96: (32, 9, 20), 128: (64, 8, 12)}[cin]
    B = 2 if cin == 72 else 1
    seed = 900 + cin + D
    x = torch.from_numpy(R.synth.normal(seed, "k333_x", (B, cin, D, H, W)))
    w = torch.from_numpy(R.synth.normal(seed, "k333_w", (cout, cin, 3, 3, 3), math.sqrt(2.0 / (27 * cout))))
    cot = R.fixture_cotangent(seed, (B, cout, D, H, W))
    out = {}
    for dt in (torch.float32, torch.float64):
        a, b = x.clone().to(dt).requires_grad_(True), w.clone().to(dt).requires_grad_(True)
        y = F.conv3d(a, b, None, 1, 1)
        y.backward(cot.to(dt))
        out[dt] = (y.detach(), a.grad, b.grad)
    A = float(F.conv3d(x.double().abs(), w.double().abs(), None, 1, 1).max())
    return x, w, cot, out, A


def _k333(cin, D, label):
    x, w, cot, out, A = conv_case(cin, D)
    xg, wg = gpu(x).requires_grad_(True), gpu(w).requires_grad_(True)
    y = ts.conv3d_k333(xg, wg)
    y.backward(gpu(cot))
    y64, gx64, gw64 = out[torch.float64]
    check("conv3d_k333 %s Cin %d D %d" % (label, cin, D), y.detach(), y64, (27 * cin + 8) * U * A)
    for name, got, want, own in (("grad_x", xg.grad, gx64, out[torch.float32][1]), ("grad_w", wg.grad, gw64, out[torch.float32][2])):
        err, bar = rel_l2(got, want), max(4 * rel_l2(own, want), 1e-6)
        report("conv3d_k333 %s Cin %d D %d %-21s rel L2 %.3e  bar %.3e  err / bar %.3f" % (label, cin, D, name, err, bar, err / bar))
        assert err <= bar, (cin, D, name)


@pytest.mark.parametrize("D", (1, 3, 5))
@pytest.mark.parametrize("cin", (72, 96, 128))
def test_conv3d_k333(cin, D):
    _k333(cin, D, "")


def test_conv3d_k333_bf16_split_form(monkeypatch):
    """the (1,3,3) launches in their x6 form (>= 32 input channels, W % 4 == 0), which small grids do not choose by themselves"""
    monkeypatch.setattr(TF, "_TRAIN_X6_MIN_GRID", 0)
    assert TF._lib.lib().ts_conv3d_hw_x6_supported(96, 32, 20, 1, 1, 0)
    _k333(96, 3, "x6")


def test_conv3d_k333_refuses_other_kernels():
    with pytest.raises(ValueError):
        ts.conv3d_k333(torch.zeros(1, 8, 2, 4, 4, device=_dev()), torch.zeros(8, 8, 1, 3, 3, device=_dev()))
    with pytest.raises(ValueError):
        ts.conv3d_k333(torch.zeros(1, 8, 2, 4, 4, device=_dev()), torch.zeros(72, 8, 3, 3, 3, device=_dev()))


# ----------------------------------------------------------------------------------------------------------------------- module
def run_module(m, x, monkeypatch):
    """-> (out, the concatenation the module built)"""
    seen = {}
    real = TF.spp3d_expand

    def spy(*a, **k):
        seen["cat"] = real(*a, **k)
        return seen["cat"]
    monkeypatch.setattr(TF, "spp3d_expand", spy)
    out = m(x)
    monkeypatch.setattr(TF, "spp3d_expand", real)
    return out, seen["cat"]


@pytest.mark.parametrize("tag", TAGS)
def test_module_against_fp64_and_the_fixture(tag, monkeypatch):
    B, C, D, H, W, training = SHAPES[tag]
    c = case(tag)
    g = R.load_fixture(tag) if tag in FIXTURES else None
    run = c["run"]
    dev = (lambda key: float(g[key])) if g is not None else None
    if g is None:           # no fixture: the deviations of spp3d_ref's own fp32 run stand in
        r32 = R.spp3d(c["x"], c["state"], STRIDES, training)
        own = dict(dev_out=float((r32["out"].double() - run["out"].detach()).abs().max()),
                   dev_cat=float((r32["cat"].double() - run["cat"].detach()).abs().max()))
        for k in run["stats"]:
            own["dev_stat_" + k] = float((r32["stats"][k].double() - run["stats"][k].double()).abs().max())
        dev = lambda key: own[key]
    m = module(tag, training)
    x = gpu(c["x"]).requires_grad_(training)
    out, cat = run_module(m, x, monkeypatch)
    out64 = run["out"].detach()
    check("module %s out" % tag, out.detach(), out64, max(4 * dev("dev_out"), 16 * U * float(out64.abs().max())))
    lv64 = run["cat"].detach()[:, C:]
    bar = max(4 * dev("dev_cat"), 16 * U * float(lv64.abs().max()))
    check("module %s cat" % tag, cat.detach()[:, C:], lv64, bar)
    assert same_bits(cat.detach()[:, :C], x.detach())
    if g is not None:
        check("module %s cat vs stored" % tag, R.sample(cat.detach()[:, C:].cpu(), g["cat_idx"]), torch.from_numpy(g["cat_val"]),
              bar + dev("dev_cat"))
        assert list(m.state_dict().keys()) == [str(k) for k in g["keys"]]
        pooled = ts.spp3d_pool(x.detach(), STRIDES)
        mean_abs = R.pool(c["x"].double().abs(), STRIDES)
        for i, (p, k) in enumerate(zip(pooled, R.boxes((D, H, W), STRIDES))):
            n = k[0] * k[1] * k[2]
            check("module %s pooled_%d vs stored" % (tag, i), p, torch.from_numpy(g["pooled_%d" % i]),
                  (n + 2) * U * mean_abs[i] + float(g["dev_pooled_%d" % i]) + 1e-300)
    if not training:
        return
    for k, want in run["stats"].items():
        got = m.state_dict()[k]
        if k.endswith("num_batches_tracked"):
            assert int(got) == int(want) == 1
        else:
            check("module %s %s" % (tag, k), got, want, max(4 * dev("dev_stat_" + k), 16 * U * float(want.abs().max())))
    out.backward(gpu(R.fixture_cotangent(seed_of(tag), out.shape)))
    want = fp64_grads(tag)
    got = {k: p.grad for k, p in m.named_parameters()}
    got["x"] = x.grad
    missed = []
    for k in sorted(want):
        if g is not None:
            own = float(g["rel_grad_" + k])
        else:
            own = None
        if own is None:
            continue
        err, bar = rel_l2(got[k], want[k]), max(4 * own, 1e-6)
        report("module %s grad %-28s rel L2 %.3e  bar %.3e  err / bar %.3f" % (tag, k, err, bar, err / bar))
        err2 = rel_l2(got[k], torch.from_numpy(g["grad_" + k]))
        report("module %s grad %-28s vs stored fp32 %.3e  bar %.3e" % (tag, k, err2, bar + own))
        if err > bar or err2 > bar + own:          # every gradient is printed before the first one fails the test
            missed.append((k, err, bar, err2, bar + own))
    assert not missed, (tag, missed)


def test_module_gradients_without_a_fixture():
    """shape f (the default in_planes), eval mode with gradients on (train mode refuses B = 1 with a one-cell level): gradients
    against fp64 autograd of spp3d_ref, the bar from spp3d_ref's own fp32 run"""
    tag = "f"
    B, C, D, H, W, _ = SHAPES[tag]
    c = case(tag)
    want = fp64_grads(tag)
    s32 = {k: (v.clone().requires_grad_("running" not in k) if v.is_floating_point() else v.clone()) for k, v in c["state"].items()}
    x32 = c["x"].clone().requires_grad_(True)
    r32 = R.spp3d(x32, s32, STRIDES, False)
    r32["out"].backward(R.fixture_cotangent(seed_of(tag), r32["out"].shape))
    own = {k: v.grad for k, v in s32.items() if v.is_floating_point() and v.grad is not None}
    own["x"] = x32.grad
    m = module(tag, False)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        module(tag, True)(gpu(c["x"]))
    x = gpu(c["x"]).requires_grad_(True)
    out = m(x)
    out.backward(gpu(R.fixture_cotangent(seed_of(tag), out.shape)))
    got = {k: p.grad for k, p in m.named_parameters()}
    got["x"] = x.grad
    for k in sorted(want):
        err, bar = rel_l2(got[k], want[k]), max(4 * rel_l2(own[k], want[k]), 1e-6)
        report("module %s grad %-28s rel L2 %.3e  bar %.3e  err / bar %.3f" % (tag, k, err, bar, err / bar))
        assert err <= bar, k


@pytest.mark.parametrize("tag", ("d", "e"))
def test_eval_under_no_grad_takes_the_folded_epilogue(tag):
    B, C, D, H, W, _ = SHAPES[tag]
    c = case(tag)
    m = module(tag, False)
    x = gpu(c["x"])
    with_grad = m(x.clone().requires_grad_(True)).detach()
    with TF.BNFolds(), torch.no_grad():
        folded = m(x)
    out64 = c["run"]["out"].detach()
    dev = float(R.load_fixture(tag)["dev_out"]) if tag in FIXTURES else \
        float((R.spp3d(c["x"], c["state"], STRIDES, False)["out"].double() - out64).abs().max())
    bar = max(4 * dev, 16 * U * float(out64.abs().max()))
    check("module %s eval, grad on" % tag, with_grad, out64, bar)
    check("module %s eval, no_grad + BNFolds" % tag, folded, out64, bar)
    check("module %s eval, folded vs grad on" % tag, folded, with_grad, bar)


def test_forward_replays_from_a_captured_graph():
    tag = "e"
    m = module(tag, False)
    x = gpu(case(tag)["x"])
    with torch.no_grad():
        eager = m(x)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m(x)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = m(x)
        captured.zero_()
        graph.replay()
        torch.cuda.synchronize()
    assert same_bits(captured, eager)


def test_train_mode_refuses_one_value_per_channel():
    m = module("d", True)
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        m(gpu(case("d")["x"]))


def test_framework_fuse_conv_agrees():
    """fuse_conv='framework' runs the 3x3x3 convolution on the framework's kernels: the same module otherwise"""
    tag = "e"
    c = case(tag)
    m = ts.SPP3D(in_planes=SHAPES[tag][1], strides=STRIDES, fuse_conv="framework")
    m.load_state_dict(c["state"], strict=True)
    m = m.to(_dev()).eval()
    out64 = c["run"]["out"].detach()
    dev = float((R.spp3d(c["x"], c["state"], STRIDES, False)["out"].double() - out64).abs().max())
    with torch.no_grad():
        check("module e fuse_conv=framework", m(gpu(c["x"])), out64, max(4 * dev, 16 * U * float(out64.abs().max())))


# ------------------------------------------------------------------------------------- BatchNorm backward, few values per channel
@pytest.mark.parametrize("act", (0, 1, 2))
@pytest.mark.parametrize("B,N", ((2, 1), (1, 3), (2, 18), (4, 1024)))
def test_bn_small_train_bwd_against_fp64(B, N, act):
    """ts_bn_small_train_bwd carries everything in fp64 up to the final rounding, so against fp64 autograd on the SAME fp32 inputs:
    |dy - dy64| <= 2 u |dy64| + 2^-40 max |g| (one rounding to fp32, doubled; the second term covers the fp64 cancellation at two values
    per channel, var / eps < 2^12 here), the two sums likewise against their own magnitudes.  Bit-equal over two runs."""
    C, eps = 16, float(np.float32(1e-5))          # the entry takes eps as fp32, like every BatchNorm entry: the expectation uses that value
    rng = np.random.RandomState(B * 7 + N + act)
    y = torch.from_numpy(rng.standard_normal((B, C, N)).astype(np.float32) * 0.2)
    g = torch.from_numpy(rng.standard_normal((B, C, N)).astype(np.float32))
    gamma = torch.from_numpy(rng.uniform(0.5, 1.5, C).astype(np.float32))
    beta = torch.from_numpy(rng.standard_normal(C).astype(np.float32) * 0.5)
    y64, ga64, be64 = (t.double().requires_grad_(True) for t in (y, gamma, beta))
    z = F.batch_norm(y64, None, None, ga64, be64, True, 0.1, eps)
    z = F.silu(z) if act == 1 else torch.relu(z) if act == 2 else z
    z.backward(g.double())
    L, st = TF._lib.lib(), TF._stream()
    runs = []
    for _ in range(2):
        yg, gg, gag, beg = gpu(y), gpu(g), gpu(gamma), gpu(beta)
        dy, s1, s2 = torch.empty_like(yg), torch.empty(C, device=_dev()), torch.empty(C, device=_dev())
        TF._lib.check(L.ts_bn_small_train_bwd(yg.data_ptr(), gg.data_ptr(), gag.data_ptr(), beg.data_ptr(), s1.data_ptr(),
                                              s2.data_ptr(), dy.data_ptr(), B, C, N, C * N, N, C * N, N, C * N, N, eps, act, st),
                      "ts_bn_small_train_bwd")
        torch.cuda.synchronize()
        runs.append((dy, s1, s2))
    assert all(same_bits(a, b) for a, b in zip(*runs))
    tiny = 2.0 ** -40 * float(g.abs().max())
    name = "bn_small B %d N %d act %d" % (B, N, act)
    check(name + " dy", runs[0][0], y64.grad, 2 * U * y64.grad.abs() + tiny)
    check(name + " sum_g", runs[0][1], be64.grad, 2 * U * be64.grad.abs() + tiny * B * N)
    check(name + " sum_gx", runs[0][2], ga64.grad, 2 * U * ga64.grad.abs() + tiny * B * N)


def test_frozen_batchnorms_run_where_train_mode_refuses():
    """a module in train() whose BatchNorms are in eval() takes running statistics: shape d runs, and equals the eval-mode module"""
    m = module("d", True)
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm3d):
            mod.eval()
    x = gpu(case("d")["x"])
    assert same_bits(m(x).detach(), module("d", False)(x).detach())


def test_conv3d_k333_inside_weight_layouts():
    """the slice layouts kept by a WeightLayouts table (a training step's): the same bits as without it, also after the weight moved
    and the table was refreshed"""
    x, w, cot, _, _ = conv_case(72, 3)
    xg, wg = gpu(x).requires_grad_(True), torch.nn.Parameter(gpu(w))

    def run():
        xg.grad, wg.grad = None, None
        y = ts.conv3d_k333(xg, wg)
        y.backward(gpu(cot))
        return y.detach().clone(), xg.grad.clone(), wg.grad.clone()
    plain = run()
    with TF.WeightLayouts() as table:
        kept = run()
        assert len(table.custom) == 6                   # three slices, forward and backward-data
        with torch.no_grad():
            wg.mul_(0.5)
        table.refresh()
        moved = run()
        assert len(table.custom) == 6
    plain_moved = run()
    assert all(same_bits(a, b) for a, b in zip(kept, plain))
    assert all(same_bits(a, b) for a, b in zip(moved, plain_moved))
    assert not same_bits(moved[0], kept[0])
