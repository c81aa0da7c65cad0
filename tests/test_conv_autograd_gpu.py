"""GPU: the HIP convolution autograd Functions (forward, backward-data, backward-weight on the matrix
cores) against torch's own conv3d / conv_transpose3d autograd on the same tensors, fp32.

Tolerances: both sides accumulate in fp32 but in different orders (ours: MFMA K-chunks / atomics);
rtol 1e-4 on outputs, and on gradients relative to the gradient's own scale."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import synth
from helpers import t

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _close(a, b, what, rtol=2e-4):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    scale = float(b.abs().max()) + 1e-12
    err = float((a - b).abs().max())
    assert err <= rtol * scale, "%s: max abs err %.3e vs scale %.3e" % (what, err, scale)


def _run(ours, ref, x, w):
    x1 = x.clone().requires_grad_(True); w1 = w.clone().requires_grad_(True)
    x2 = x.clone().requires_grad_(True); w2 = w.clone().requires_grad_(True)
    y1, y2 = ours(x1, w1), ref(x2, w2)
    assert y1.shape == y2.shape
    _close(y1, y2, "forward")
    g = t(synth.normal(77, "g", tuple(y2.shape)), x.device)
    y1.backward(g); y2.backward(g)
    _close(x1.grad, x2.grad, "grad input")
    _close(w1.grad, w2.grad, "grad weight")


@pytest.mark.parametrize("cin,cout,stride,dil,shape", [
    (24, 8, 1, 1, (2, 5, 21, 37)), (16, 32, 2, 1, (2, 3, 20, 36)), (16, 32, 2, 1, (1, 3, 17, 31)),   # odd sizes: cropped transposed form
    (8, 16, 1, 2, (2, 4, 19, 33)), (40, 64, 1, 1, (1, 2, 9, 15)), (304, 8, 1, 1, (1, 5, 17, 40)),
    (64, 64, 2, 1, (1, 6, 17, 30))])
def test_conv_hw_autograd(cin, cout, stride, dil, shape):
    import temporalstereo_amd.functional as TF
    dev = _dev()
    B, D, H, W = shape
    x = t(synth.normal(1, "x", (B, cin, D, H, W)), dev)
    w = t(synth.normal(2, "w", (cout, cin, 1, 3, 3), 0.1), dev)
    s, p, d = (1, stride, stride), (0, dil, dil), (1, dil, dil)
    assert TF.conv3d_supported(tuple(w.shape), s, p, d, 1) == "hw"
    _run(lambda a, b: TF.conv3d(a, b, None, s, p, d), lambda a, b: F.conv3d(a, b, None, s, p, d), x, w)


@pytest.mark.parametrize("k,stride,dil,pad,din", [(3, 1, 1, 1, 7), (3, 2, 1, 1, 7), (3, 2, 1, 1, 12), (3, 1, 2, 2, 9), (5, 1, 1, 2, 14), (1, 1, 1, 0, 5)])
def test_conv_d_autograd(k, stride, dil, pad, din):
    import temporalstereo_amd.functional as TF
    dev = _dev()
    x = t(synth.normal(3, "x", (2, 16, din, 11, 23)), dev)
    w = t(synth.normal(4, "w", (32, 16, k, 1, 1), 0.2), dev)
    s, p, d = (stride, 1, 1), (pad, 0, 0), (dil, 1, 1)
    assert TF.conv3d_supported(tuple(w.shape), s, p, d, 1) == "d"
    _run(lambda a, b: TF.conv3d(a, b, None, s, p, d), lambda a, b: F.conv3d(a, b, None, s, p, d), x, w)


def test_conv_transpose_autograd_both_families():
    import temporalstereo_amd.functional as TF
    dev = _dev()
    x = t(synth.normal(5, "x", (2, 32, 3, 9, 15)), dev)
    w = t(synth.normal(6, "w", (32, 16, 1, 3, 3), 0.1), dev)
    a = ((1, 2, 2), (0, 1, 1), (0, 1, 1))
    _run(lambda u, v: TF.conv_transpose3d(u, v, None, *a), lambda u, v: F.conv_transpose3d(u, v, None, a[0], a[1], a[2]), x, w)
    w = t(synth.normal(7, "w", (32, 16, 3, 1, 1), 0.1), dev)
    a = ((2, 1, 1), (1, 0, 0), (1, 0, 0))
    _run(lambda u, v: TF.conv_transpose3d(u, v, None, *a), lambda u, v: F.conv_transpose3d(u, v, None, a[0], a[1], a[2]), x, w)


def test_layers_use_the_hip_convolutions_on_gpu():
    """layers.Conv3d / ConvTranspose3d: same numbers whichever backend runs the convolution, and the HIP
    backend really is the one that runs (its autograd node is ours)."""
    from temporalstereo_amd import layers
    dev = _dev()
    torch.manual_seed(0)
    m = layers.Conv3d(16, 8, (1, 3, 3), (1, 1, 1), (0, 1, 1), bias=True, norm=('BN3d', 8), activation='SiLU').to(dev).train()
    x = t(synth.normal(8, "x", (2, 16, 4, 12, 20)), dev).requires_grad_(True)
    y = m(x)
    names, todo = set(), [y.grad_fn]
    while todo:
        fn = todo.pop()
        if fn is not None:
            names.add(type(fn).__name__)
            todo += [f for f, _ in fn.next_functions]
    # conv -> BatchNorm -> SiLU is ONE node of ours (functional._ConvBNAct); nothing of the framework's in between
    assert names <= {"_ConvBNActBackward", "AccumulateGrad"} and "_ConvBNActBackward" in names, names
    y.square().mean().backward()
    g_hip = m.weight.grad.clone(); gx_hip = x.grad.clone()
    m.zero_grad(); x.grad = None
    layers.set_conv_backend("torch")
    try:
        y2 = m(x)
        y2.square().mean().backward()
    finally:
        layers.set_conv_backend("hip")
    _close(y, y2, "layer forward")
    _close(g_hip, m.weight.grad, "layer grad weight")
    _close(gx_hip, x.grad, "layer grad input")
    # unsupported hyper-parameters fall back to the framework convolution instead of failing
    odd = layers.Conv3d(4, 4, (3, 3, 3), padding=1).to(dev)
    assert odd(torch.zeros(1, 4, 3, 5, 5, device=dev)).shape == (1, 4, 3, 5, 5)


def _graph_nodes(y):
    """Names of the autograd nodes behind y, one per node, without the leaves' AccumulateGrad."""
    names, seen, todo = [], set(), [y.grad_fn]
    while todo:
        fn = todo.pop()
        if fn is not None and fn not in seen:
            seen.add(fn)
            names.append(type(fn).__name__)
            todo += [f for f, _ in fn.next_functions]
    return sorted(n for n in names if n != "AccumulateGrad")


@pytest.mark.parametrize("family", ["hw", "d", "dc", "hw3"])
def test_each_family_is_one_autograd_node(family):
    """The raw public function of each family puts exactly ONE node of ours into the graph (functional._ConvRaw), the fused wrapper
    exactly _ConvBNAct.  conv3d / conv_transpose3d of the (1,3,3) family and conv_transpose3d of the (k,1,1) family add their bias with
    the framework's add behind the node (a view of the bias and the add: nothing else); the others carry it in the kernel's epilogue."""
    import temporalstereo_amd.functional as TF
    dev = _dev()
    ours = "_ConvRawBackward"
    outside = sorted([ours, "AddBackward0", "ViewBackward0"])
    leaf = lambda seed, shape, scale=1.0: t(synth.normal(seed, "v", shape, scale), dev).requires_grad_(True)
    if family == "hw":
        x, w, wt, b = leaf(1, (1, 40, 2, 9, 15)), leaf(2, (64, 40, 1, 3, 3), 0.1), leaf(3, (40, 64, 1, 3, 3), 0.1), leaf(4, (64,))
        s, p, d, tr = (1, 1, 1), (0, 1, 1), (1, 1, 1), ((1, 2, 2), (0, 1, 1), (0, 1, 1))
        raw = [(TF.conv3d(x, w, None, s, p, d), [ours]), (TF.conv3d(x, w, b, s, p, d), outside),
               (TF.conv_transpose3d(x, wt, None, *tr), [ours]), (TF.conv_transpose3d(x, wt, b, *tr), outside)]
        geom = (1, 1, False)
    elif family == "d":
        x, w, wt, b = leaf(1, (2, 16, 5, 11, 23)), leaf(2, (32, 16, 3, 1, 1), 0.2), leaf(3, (16, 32, 3, 1, 1), 0.2), leaf(4, (32,))
        s, p, d, tr = (1, 1, 1), (1, 0, 0), (1, 1, 1), ((2, 1, 1), (1, 0, 0), (1, 0, 0))
        raw = [(TF.conv3d(x, w, None, s, p, d), [ours]), (TF.conv3d(x, w, b, s, p, d), [ours]),          # bias in the epilogue
               (TF.conv_transpose3d(x, wt, None, *tr), [ours]), (TF.conv_transpose3d(x, wt, b, *tr), outside)]
        geom = (1, 1, 1, False)
    elif family == "dc":
        x, w, b = leaf(1, (2, 8, 5, 7)), leaf(2, (8, 16, 4, 4), 0.1), leaf(4, (16,))
        raw = [(TF.conv_transpose2d_k4s2(x, w), [ours]), (TF.conv_transpose2d_k4s2(x, w, b), [ours])]
        geom = None
    else:
        x, w, b = leaf(1, (2, 8, 1, 5, 7)), leaf(2, (8, 8, 3, 3, 3), 0.1), leaf(4, (8,))
        raw = [(TF.conv3d_k333(x, w), [ours])]
        geom = (1, 1, False)
    for y, want in raw:
        assert _graph_nodes(y) == want
    cout = b.numel()
    bn = (torch.nn.BatchNorm2d(cout) if family == "dc" else torch.nn.BatchNorm3d(cout)).to(dev).train()
    y = TF.conv_bn_act(x, w, b, bn, "SiLU", family, geom)
    assert _graph_nodes(y) == ["_ConvBNActBackward"]
    y.sum().backward()
    assert all(v.grad is not None for v in (x, w, b, bn.weight, bn.bias))


# ------------------------------------------------------------------------------- element stages
def test_resize_add_silu_autograd():
    import temporalstereo_amd.functional as TF
    dev = _dev()
    for (sa, sb) in (((2, 6, 3, 9, 15), (2, 6, 5, 17, 30)), ((1, 4, 6, 18, 30), (1, 4, 6, 17, 30)), ((2, 3, 2, 5, 7), (2, 3, 2, 5, 7))):
        a = t(synth.normal(11, "a", sa), dev); b = t(synth.normal(12, "b", sb), dev)
        a1, b1 = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
        a2, b2 = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
        y1 = TF.resize_add_silu(a1, b1)
        y2 = F.silu(F.interpolate(a2, size=sb[2:], mode="trilinear", align_corners=True) + b2)
        _close(y1, y2, "forward", 1e-5)
        g = t(synth.normal(13, "g", sb), dev)
        y1.backward(g); y2.backward(g)
        _close(a1.grad, a2.grad, "grad a")
        _close(b1.grad, b2.grad, "grad add", 1e-5)


def test_pool5_avgmax_autograd():
    import temporalstereo_amd.functional as TF
    dev = _dev()
    x = t(synth.normal(21, "x", (2, 5, 7, 19, 41)), dev)
    x1, x2 = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    a1, m1 = TF.pool5_avgmax(x1)
    a2, m2 = F.avg_pool3d(x2, 5, 1, 2), F.max_pool3d(x2, 5, 1, 2)
    _close(a1, a2, "avg", 1e-5); _close(m1, m2, "max", 0.0)
    ga, gm = t(synth.normal(22, "ga", tuple(x.shape)), dev), t(synth.normal(23, "gm", tuple(x.shape)), dev)
    (a1 * ga + m1 * gm).sum().backward(); (a2 * ga + m2 * gm).sum().backward()
    _close(x1.grad, x2.grad, "grad x")


def test_sort_gather_autograd_is_the_stable_sort():
    import temporalstereo_amd.functional as TF
    dev = _dev()
    B, C, DT, H, W = 2, 6, 14, 9, 13
    vol = t(synth.normal(31, "v", (B, C, DT, H, W)), dev)
    smp = t(synth.normal(32, "s", (B, DT, H, W)), dev)
    smp[:, 3] = smp[:, 0]; smp[:, 12:] = 0.0; smp[:, 5, :4] = 0.0          # ties: stable order must hold
    v1, s1 = vol.clone().requires_grad_(True), smp.clone().requires_grad_(True)
    v2, s2 = vol.clone().requires_grad_(True), smp.clone().requires_grad_(True)
    ov1, os1 = TF.sort_gather(v1, s1)
    os2, order = torch.sort(s2, dim=1, stable=True)
    ov2 = torch.gather(v2, 2, order.unsqueeze(1).expand(-1, C, -1, -1, -1))
    assert torch.equal(os1, os2) and torch.equal(ov1, ov2)
    gv, gs = t(synth.normal(33, "gv", tuple(vol.shape)), dev), t(synth.normal(34, "gs", tuple(smp.shape)), dev)
    ((ov1 * gv).sum() + (os1 * gs).sum()).backward(); ((ov2 * gv).sum() + (os2 * gs).sum()).backward()
    assert torch.equal(v1.grad, v2.grad) and torch.equal(s1.grad, s2.grad)


@pytest.mark.parametrize("case", range(10))
def test_fused_conv_batchnorm_activation_matches_framework(case):
    """layers.Conv3d / ConvTranspose3d / Conv2d with BatchNorm + activation: the fused HIP node (functional.conv_bn_act: own
    statistics / normalise+activate / backward kernels) against the same module on the framework's convolution, BatchNorm and
    activation -- outputs, all five gradients and the running statistics, train and eval mode."""
    import copy
    from temporalstereo_amd import layers
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(40 + case)
    act = [None, "SiLU", "ReLU"][case % 3]
    train = case % 4 != 3
    B = int(rng.choice([1, 2, 3]))
    kind = ["hw", "hw_s2", "hw_d2", "d3", "d5", "d_s2", "hwT", "dT", "2d", "2d_s2"][case]
    cin, cout = int(rng.choice([3, 8, 16])), int(rng.choice([4, 8, 32]))
    D, H, W = int(rng.randint(2, 6)), int(rng.randint(5, 20)), int(rng.randint(6, 40))
    bias = bool(case % 2)
    if kind in ("2d", "2d_s2"):
        m = layers.Conv2d(cin, cout, 3, 2 if kind == "2d_s2" else 1, 1, bias=bias, norm=("BN", cout), activation=act)
        x = torch.from_numpy(synth.normal(60 + case, "x", (B, cin, H, W)))
    elif kind == "hwT":
        m = layers.ConvTranspose3d(cin, cout, (1, 3, 3), (1, 2, 2), (0, 1, 1), (0, 1, 1), bias=bias, norm=("BN3d", cout), activation=act)
        x = torch.from_numpy(synth.normal(60 + case, "x", (B, cin, D, H, W)))
    elif kind == "dT":
        m = layers.ConvTranspose3d(cin, cout, (3, 1, 1), (2, 1, 1), (1, 0, 0), (1, 0, 0), bias=bias, norm=("BN3d", cout), activation=act)
        x = torch.from_numpy(synth.normal(60 + case, "x", (B, cin, D, H, W)))
    else:
        args = {"hw": ((1, 3, 3), (1, 1, 1), (0, 1, 1), (1, 1, 1)), "hw_s2": ((1, 3, 3), (1, 2, 2), (0, 1, 1), (1, 1, 1)),
                "hw_d2": ((1, 3, 3), (1, 1, 1), (0, 2, 2), (1, 2, 2)), "d3": ((3, 1, 1), (1, 1, 1), (1, 0, 0), (1, 1, 1)),
                "d5": ((5, 1, 1), (1, 1, 1), (2, 0, 0), (1, 1, 1)), "d_s2": ((3, 1, 1), (2, 1, 1), (1, 0, 0), (1, 1, 1))}[kind]
        m = layers.Conv3d(cin, cout, args[0], args[1], args[2], args[3], bias=bias, norm=("BN3d", cout), activation=act)
        x = torch.from_numpy(synth.normal(60 + case, "x", (B, cin, D, H, W)))
    with torch.no_grad():
        m.norm.weight.copy_(torch.from_numpy(synth.uniform(60 + case, "g", (cout,), 0.5, 1.5)))
        m.norm.bias.copy_(torch.from_numpy(synth.normal(60 + case, "b", (cout,), 0.2)))
        m.norm.running_mean.copy_(torch.from_numpy(synth.normal(60 + case, "rm", (cout,), 0.2)))
        m.norm.running_var.copy_(torch.from_numpy(synth.uniform(60 + case, "rv", (cout,), 0.5, 1.5)))
    m = m.to(dev).train(train)
    # the arbiter is the same module in fp64 on the framework's ops: the framework's own fp32 BatchNorm / strided-convolution
    # backward is 1-6 % off the fp64 result on some of these geometries (tools/exp/dbg_bn.py: d_s2, B=3), ours 1e-7
    ref = copy.deepcopy(m).double()
    xa, xb = x.to(dev).requires_grad_(True), x.to(dev).double().requires_grad_(True)
    ya = m(xa)
    layers.set_conv_backend("torch")
    try:
        yb = ref(xb)
    finally:
        layers.set_conv_backend("hip")
    g = torch.from_numpy(synth.normal(70 + case, "gy", tuple(yb.shape))).to(dev)
    ya.backward(g)
    yb.backward(g.double())
    tag = "%s act=%s train=%s" % (kind, act, train)
    rel = lambda a, b: float((a.double() - b).abs().max()) / (float(b.abs().max()) + 1e-9)
    assert rel(ya.detach(), yb.detach()) < 5e-6, tag
    for (na, pa), (_, pb) in zip([("x", xa)] + list(m.named_parameters()), [("x", xb)] + list(ref.named_parameters())):
        if na == "bias" and train:          # BatchNorm removes the mean: the true gradient is 0; ours is rounding noise around it
            assert float(pa.grad.abs().max()) <= 1e-4 * float(g.abs().sum()), "%s grad bias" % tag
            continue
        assert rel(pa.grad, pb.grad) < 2e-5, "%s grad %s: %.3g" % (tag, na, rel(pa.grad, pb.grad))
    for k in ("running_mean", "running_var"):
        a, b = getattr(m.norm, k), getattr(ref.norm, k)
        assert rel(a, b) < 1e-5, "%s %s" % (tag, k)
    assert int(m.norm.num_batches_tracked) == int(ref.norm.num_batches_tracked)


def test_batchnorm_two_launch_form_equals_the_three_launch_form(monkeypatch):
    """Single-rank training uses ts_bn_train_{fwd,bwd} (the normalise / input-gradient kernels finish their channel's partial sums
    themselves); the SyncBatchNorm path exchanges the statistics between ts_bn_stats_fwd / ts_bn_apply_act_fwd and between
    ts_bn_act_bwd_reduce / _apply.  Same partials, same fixed summation order: outputs, gradients and running statistics must be
    identical to the bit."""
    import copy
    from temporalstereo_amd import functional as TF, layers, _lib
    dev = torch.device("cuda:0")
    res = {}
    old = _lib.lib().ts_bn_set_small_elems(0)           # (this layer is small enough for the one-launch form, tested below)
    for fused in (True, False):
        monkeypatch.setattr(TF, "_BN_FUSED", fused)
        torch.manual_seed(3)
        m = layers.Conv3d(16, 24, (1, 3, 3), (1, 1, 1), (0, 1, 1), (1, 1, 1), bias=False, norm=("BN3d", 24), activation="SiLU").to(dev).train()
        x = torch.from_numpy(synth.normal(91, "x", (2, 16, 3, 21, 36))).to(dev).requires_grad_(True)
        y = m(x)
        y.backward(torch.from_numpy(synth.normal(92, "g", tuple(y.shape))).to(dev))
        res[fused] = [y.detach(), x.grad, m.weight.grad, m.norm.weight.grad, m.norm.bias.grad, m.norm.running_mean.clone(),
                      m.norm.running_var.clone(), m.norm.num_batches_tracked.clone()]
    _lib.lib().ts_bn_set_small_elems(old)
    for a, b in zip(res[True], res[False]):
        assert torch.equal(a, b)
    assert int(res[True][-1]) == 1


@pytest.mark.parametrize("shape", [(2, 16, 3, 21, 36), (1, 24, 2, 17, 30), (1, 8, 1, 9, 15), (3, 5, 1, 7, 11)])
def test_batchnorm_one_launch_form_for_small_layers(shape):
    """Channels of at most ts_bn_set_small_elems() elements take ONE launch each way (a workgroup per channel: sums, then the
    normalisation / input gradient): against the two-launch form to rounding, and against float64 framework ops like the fused node
    itself (reference behaviour: conv -> nn.BatchNorm3d -> SiLU in train mode, layers/basic_layers.py:194-235)."""
    from temporalstereo_amd import layers, _lib
    dev = torch.device("cuda:0")
    B, C, D, H, W = shape
    res = {}
    L = _lib.lib()
    old = L.ts_bn_set_small_elems(-1)
    assert B * D * H * W <= old, "default bound moved: pick smaller shapes"
    try:
        for cap in (old, 0):
            L.ts_bn_set_small_elems(cap)
            torch.manual_seed(5)
            m = layers.Conv3d(C, C + 3, (1, 3, 3), (1, 1, 1), (0, 1, 1), (1, 1, 1), bias=False, norm=("BN3d", C + 3), activation="SiLU").to(dev).train()
            with torch.no_grad():
                m.norm.weight.uniform_(0.5, 1.5); m.norm.bias.normal_(0, 0.3)
            x = torch.from_numpy(synth.normal(191, "x", shape)).to(dev).requires_grad_(True)
            y = m(x)
            y.backward(torch.from_numpy(synth.normal(192, "g", tuple(y.shape))).to(dev))
            res[cap] = [y.detach(), x.grad, m.weight.grad, m.norm.weight.grad, m.norm.bias.grad, m.norm.running_mean.clone(), m.norm.running_var.clone()]
            last = m
    finally:
        L.ts_bn_set_small_elems(old)
    rel = lambda a, b: float((a.double() - b.double()).abs().max()) / (float(b.double().abs().max()) + 1e-12)
    for a, b in zip(res[old], res[0]):
        assert rel(a, b) < 2e-6
    # float64 framework ops on the same weights
    ref = torch.nn.Sequential(torch.nn.Conv3d(C, C + 3, (1, 3, 3), 1, (0, 1, 1), bias=False), torch.nn.BatchNorm3d(C + 3), torch.nn.SiLU()).double().to(dev).train()
    with torch.no_grad():
        ref[0].weight.copy_(last.weight.double()); ref[1].weight.copy_(last.norm.weight.double()); ref[1].bias.copy_(last.norm.bias.double())
    xd = torch.from_numpy(synth.normal(191, "x", shape)).to(dev).double().requires_grad_(True)
    yd = ref(xd)
    yd.backward(torch.from_numpy(synth.normal(192, "g", tuple(yd.shape))).to(dev).double())
    want = [yd.detach(), xd.grad, ref[0].weight.grad, ref[1].weight.grad, ref[1].bias.grad]
    for a, b in zip(res[old][:5], want):
        assert rel(a, b) < 2e-5


def test_wgrad_defer_survives_an_aborted_step():
    """functional.WgradDefer: a step that raises between the first deferred weight-gradient call and flush() must not
    leave descriptors behind -- the next step's finish launch would write old partial sums through pointers to freed memory.  An
    aborted step, then a clean one: the clean one's gradient equals torch's; and a weight that already has a .grad (autograd would
    ACCUMULATE into the still-unwritten tensor) is not deferred."""
    import temporalstereo_amd.functional as TF
    from temporalstereo_amd import _lib
    dev = _dev()
    x = t(synth.normal(5, "x", (1, 16, 2, 12, 32)), dev)
    w = t(synth.normal(6, "w", (16, 16, 1, 3, 3), 0.1), dev).requires_grad_(True)
    s, p, d = (1, 1, 1), (0, 1, 1), (1, 1, 1)
    defer = TF.WgradDefer()

    class Boom(RuntimeError):
        pass

    class _Raise(torch.autograd.Function):
        @staticmethod
        def forward(ctx, a):
            return a.clone()

        @staticmethod
        def backward(ctx, g):
            raise Boom("mid-backward")

    L = _lib.lib()
    with pytest.raises(Boom):
        with defer:
            xin = x.clone().requires_grad_(True)
            y = TF.conv3d(_Raise.apply(xin), w, None, s, p, d)       # the conv's weight gradient is deferred, then the input's path raises
            y.sum().backward()
    assert int(L.ts_conv_wgrad_pending()) == 0 and defer.keep == [], "an aborted step left deferred finishes behind"
    w.grad = None
    with defer:
        y = TF.conv3d(x, w, None, s, p, d)
        y.sum().backward()
        defer.flush()
    w2 = w.detach().clone().requires_grad_(True)
    F.conv3d(x, w2, None, s, p, d).sum().backward()
    _close(w.grad, w2.grad, "weight gradient of the clean step")
    # a second backward into the SAME .grad: accumulated by autograd, so it must take the immediate finish
    with defer:
        y = TF.conv3d(x, w, None, s, p, d)
        y.sum().backward()
        assert int(L.ts_conv_wgrad_pending()) == 0, "a weight with a gradient already in place was deferred"
        defer.flush()
    torch.cuda.synchronize()
    _close(w.grad, 2 * w2.grad, "accumulated weight gradient")
