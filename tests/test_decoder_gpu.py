"""FeatureDecoder on the device (temporalstereo_amd.FeatureDecoder / functional.decoder_conv; csrc/feature_decoder.hip) against the
reference's own runs recorded in tests/golden/decoder_*.npz (tools/gen_golden.py --only-decoder) and against tests/decoder_ref.py in fp64
on the CPU.  u = 2^-24.

Bars, none taken from the code under test (the project's convention; the factor 4 is argued in tests/test_raft_corr_gpu.py):
  stages and outputs   |hip - fp64| <= max(4 x dev_stage, 16 u max |stage|), dev_stage = max |fp32 run - fp64 run| of the reference on the
                       CPU: the fixture's, and for the shapes without a fixture (the single layers, the range and routing cases) the same
                       figure from an fp32 and an fp64 run of decoder_ref inside the test.
  gradients            against fp64: relative L2 <= max(4 x rel_grad_key, 1e-6); against the stored fp32 gradients (at the stored
                       positions): that plus rel_grad_key (triangle inequality).
Each case prints error / bar; with TS_DECODER_PARITY_FILE set the line is appended to that file (profiles/decoder_parity.txt is made so).
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn

import decoder_ref as R
import synth
from compare import Parity, dev as _dev, gpu, same_bits, stage_bar
import temporalstereo_amd as ts
from temporalstereo_amd import _lib
from temporalstereo_amd import functional as TF
from temporalstereo_amd import layers

pytestmark = pytest.mark.gpu

P = Parity("TS_DECODER_PARITY_FILE")
check, check_rel = P.check, P.check_rel
#         tag        B  Cu   Cs   Cout  h  w   H   W
LAYERS = {"ragged": (2, 12, 5, 20, 4, 7, 9, 13),            # nothing a multiple of a tile; the source seam inside a K chunk
          "deconv32_16": (1, 320, 160, 256, 2, 3, 3, 5),    # that layer's own widths, K = 4320
          "conv32": (2, 0, 272, 320, 0, 0, 3, 5),           # the plain form
          "long_row": (1, 128, 48, 64, 5, 9, 10, 70),       # a row longer than a tile, ratio 2 down and 7.67 across
          "one_row": (1, 16, 3, 33, 1, 6, 2, 130),          # h = 1: the vertical step is 0; Cout one past a 32-wide tile
          "centre": (1, 8, 8, 8, 1, 1, 1, 1),               # only the centre tap is live (forward only, eval statistics)
          "identity": (1, 4, 4, 16, 6, 6, 6, 6)}            # the resize is the identity
LAYER_TAGS = tuple(LAYERS)
FIXTURES = ("a", "b")


# ------------------------------------------------------------------------------------------------------------------ one fused layer
def layer_inputs(tag, dtype=torch.float32, weight_scale=1.0):
    """Seeded inputs of one fused layer: dict(up, skip, weight, gamma, beta, mean, var, cot)."""
    B, Cu, Cs, Cout, h, w, H, W = LAYERS[tag]
    seed = 7100 + sum(map(ord, tag))
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32)).to(dtype)
    Cin = Cu + Cs
    weight = synth.normal(seed, "w", (Cout, Cin, 3, 3)).astype(np.float64) * (2.0 * weight_scale / np.sqrt(9.0 * Cin))
    return dict(up=t(synth.normal(seed, "up", (B, Cu, h, w))) if Cu else None, skip=t(synth.normal(seed, "skip", (B, Cs, H, W))),
                weight=t(weight), gamma=t(synth.uniform(seed, "gamma", (Cout,), 0.5, 1.5)), beta=t(synth.normal(seed, "beta", (Cout,), 0.1)),
                mean=t(synth.normal(seed, "mean", (Cout,), 0.1)), var=t(synth.uniform(seed, "var", (Cout,), 0.5, 1.5)),
                cot=R.cotangent(seed, "layer", (B, Cout, H, W), dtype))


LAYER_GRADS = ("up", "skip", "weight", "gamma", "beta")


def layer_ref(tag, dtype, weight_scale=1.0):
    """decoder_ref's fused layer (BatchNorm, SiLU) in `dtype`: dict(out, grad_*); train statistics unless the plane is 1 x 1."""
    a = layer_inputs(tag, dtype, weight_scale)
    training = tag != "centre"
    for k in LAYER_GRADS:
        if a[k] is not None and training:
            a[k].requires_grad_(True)
    bn = dict(weight=a["gamma"], bias=a["beta"], running_mean=a["mean"], running_var=a["var"])
    out = R.fused_layer(a["up"], a["skip"], a["weight"], None, bn, "SiLU", training)
    res = dict(out=out.detach())
    if training:
        out.backward(a["cot"])
        for k in LAYER_GRADS:
            if a[k] is not None:
                res["grad_" + k] = a[k].grad.detach()
    return res


@functools.lru_cache(maxsize=None)
def layer_case(tag, weight_scale=1.0):
    """The fp64 run and the deviations the bars are made of, computed once and left unchanged."""
    r64, r32 = layer_ref(tag, torch.float64, weight_scale), layer_ref(tag, torch.float32, weight_scale)
    dev = float((r32["out"].double() - r64["out"]).abs().max())
    rel = {k[5:]: float((r32[k].double() - r64[k]).norm() / r64[k].norm()) for k in r64 if k.startswith("grad_")}
    return dict(r64=r64, dev=dev, rel=rel)


def layer_module(a, training):
    bn = nn.BatchNorm2d(a["gamma"].numel())
    with torch.no_grad():
        bn.weight.copy_(a["gamma"]); bn.bias.copy_(a["beta"]); bn.running_mean.copy_(a["mean"]); bn.running_var.copy_(a["var"])
    return bn.to(_dev()).train(training)


def layer_device(tag, weight_scale=1.0, plain_on_cat=False):
    """functional.decoder_conv on the device -> dict(out, grad_*)"""
    a = layer_inputs(tag, weight_scale=weight_scale)
    training = tag != "centre"
    bn = layer_module(a, training)
    up, skip, weight = (gpu(a[k]).requires_grad_(training) if a[k] is not None else None for k in ("up", "skip", "weight"))
    if plain_on_cat:
        out = TF.decoder_conv(None, torch.cat([up, skip], 1), weight, None, bn, "SiLU")
    else:
        out = TF.decoder_conv(up, skip, weight, None, bn, "SiLU")
    res = dict(out=out.detach())
    if training:
        out.backward(gpu(a["cot"]))
        for k, t in (("up", up), ("skip", skip), ("weight", weight), ("gamma", bn.weight), ("beta", bn.bias)):
            if t is not None:
                res["grad_" + k] = t.grad
    return res


@pytest.mark.parametrize("tag", LAYER_TAGS)
def test_one_layer(tag):
    c = layer_case(tag)
    got = layer_device(tag)
    want = c["r64"]
    bar = stage_bar(c["dev"], float(want["out"].abs().max()))
    check("layer %s out" % tag, got["out"], want["out"], bar)
    assert set(got) == set(want)
    for k in c["rel"]:
        check_rel("layer %s grad %s" % (tag, k), got["grad_" + k], want["grad_" + k], want["grad_" + k], max(4.0 * c["rel"][k], 1e-6))
    if tag == "identity":           # the resize is the identity: the fused form against the plain form on torch.cat
        plain = layer_device(tag, plain_on_cat=True)
        check("layer identity out (fused - plain on torch.cat)", got["out"], plain["out"], bar)


def test_plain_layer_with_a_bias_and_no_norm():
    """No BatchNorm, no activation, a bias (none of the decoder's layers has one; the functional form does): out and four gradients."""
    B, Cu, Cs, Cout, h, w, H, W = LAYERS["ragged"]
    a = layer_inputs("ragged")

    def ref(dt):
        t = {k: a[k].to(dt).clone().requires_grad_(True) for k in ("up", "skip", "weight", "beta")}
        out = R.fused_layer(t["up"], t["skip"], t["weight"], t["beta"])
        out.backward(a["cot"].to(dt))
        return dict(out=out.detach(), **{"grad_" + k: v.grad for k, v in t.items()})
    r64, r32 = ref(torch.float64), ref(torch.float32)
    t = {k: gpu(a[k]).requires_grad_(True) for k in ("up", "skip", "weight", "beta")}
    out = TF.decoder_conv(t["up"], t["skip"], t["weight"], t["beta"])
    out.backward(gpu(a["cot"]))
    check("plain layer out", out.detach(), r64["out"], stage_bar(float((r32["out"].double() - r64["out"]).abs().max()), float(r64["out"].abs().max())))
    for k in t:
        rel = float((r32["grad_" + k].double() - r64["grad_" + k]).norm() / r64["grad_" + k].norm())
        check_rel("plain layer grad %s" % ("bias" if k == "beta" else k), t[k].grad, r64["grad_" + k], r64["grad_" + k], max(4.0 * rel, 1e-6))


def test_weights_scaled_by_1e3():
    c = layer_case("ragged", 1e3)
    got = layer_device("ragged", 1e3)
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    check("layer ragged, weights x 1e3, out", got["out"], c["r64"]["out"], stage_bar(c["dev"], float(c["r64"]["out"].abs().max())))
    for k in c["rel"]:
        check_rel("layer ragged, weights x 1e3, grad %s" % k, got["grad_" + k], c["r64"]["grad_" + k], c["r64"]["grad_" + k],
                  max(4.0 * c["rel"][k], 1e-6))


def test_bits_do_not_depend_on_the_batch_grouping():
    """Sixteen images of Cu = 24 (from a 13 x 27 map), Cs = 20 on a 31 x 63 plane, a bias, no BatchNorm: Cin = 44 is six chunks (one
    flush of the blocked summation is crossed, the source seam inside a chunk, a ragged last chunk), 32 pixel tiles per image, ragged
    at the right and the bottom.  The calls of every grouping have the bits of the B = 16 call.  The launch rule (csrc/conv_hw3.hpp
    launch_rule, at least 512 workgroups) sends the groupings to
        (a) Cout = 128   B = 16  decoder_conv_kernel<8>    B = 8  <4>    B = 4  <2>    B = 2  <1>
        (b) Cout = 130   B = 16  decoder_conv_kernel<8>, two row groups, the second with 2 live rows of 128    B = 2  <1>
    -- every instantiation there is, where no LAYERS entry leaves <1>.  Observed in a kernel trace of this test (rocprofv3
    --kernel-trace, a run of its own): profiles/hw3_grouping_kernel_trace.txt.  The B = 2 result also meets the fp64 restatement at
    the stage bar."""
    B, Cu, Cs, h, w, H, W = 16, 24, 20, 13, 27, 31, 63
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))
    for Cout, groupings in ((128, (16, 8, 4, 2)), (130, (16, 2))):
        seed = 7100 + Cout
        up, skip = t(synth.normal(seed, "up", (B, Cu, h, w))), t(synth.normal(seed, "skip", (B, Cs, H, W)))
        weight = t(synth.normal(seed, "w", (Cout, Cu + Cs, 3, 3)).astype(np.float64) * (2.0 / np.sqrt(9.0 * (Cu + Cs))))
        bias = t(synth.normal(seed, "bias", (Cout,), 0.1))
        ud, sd, wd, bd = gpu(up), gpu(skip), gpu(weight), gpu(bias)

        def grouped(n):
            with torch.no_grad():
                return torch.cat([TF.decoder_conv(ud[i:i + n], sd[i:i + n], wd, bd) for i in range(0, B, n)])
        whole = grouped(groupings[0])
        for n in groupings[1:]:
            got = grouped(n)
            assert same_bits(got, whole), "Cout = %d, B = %d" % (Cout, n)
        assert n == 2
        r64 = R.fused_layer(up[:2].double(), skip[:2].double(), weight.double(), bias.double())
        r32 = R.fused_layer(up[:2], skip[:2], weight, bias)
        check("grouping, Cout = %d, B = 2, first call" % Cout, got[:2], r64, stage_bar(float((r32.double() - r64).abs().max()), float(r64.abs().max())))


# ------------------------------------------------------------------------------------------------------------------ the module
GRADS = R.INPUTS + R.PARAM_KEYS


@functools.lru_cache(maxsize=None)
def case(tag, mode):
    g = R.load_fixture(tag)
    return dict(g=g, seed=g["seed"], r64=R.run(g["seed"], tag, torch.float64, mode == "train"))


def module_for(seed, training):
    m = ts.FeatureDecoder()
    m.load_state_dict(R.fixture_state(seed), strict=True)
    return m.to(_dev()).train(training)


def device_run(tag, mode, maps=None, backward=True):
    """ts.FeatureDecoder on the fixture's inputs -> dict(x4, x8, x16, grad_*)"""
    c = case(tag, mode)
    m = module_for(c["seed"], mode == "train")
    own = maps is None
    if own:
        maps = {k: gpu(v).requires_grad_(backward) for k, v in R.fixture_input(c["seed"], tag).items()}
    outs = m(maps["x4"], maps["x8"], maps["x16"], maps["x32"])
    res = {k: v.detach() for k, v in zip(R.OUTPUTS, outs)}
    if backward:
        cots = R.fixture_cotangents(c["seed"], tag)
        torch.autograd.backward(list(outs), [gpu(cots[k]) for k in R.OUTPUTS])
        if own:
            for k in R.INPUTS:
                res["grad_" + k] = maps[k].grad
        for k, p in m.named_parameters():
            res["grad_" + k] = p.grad
    return res


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("tag", FIXTURES)
def test_fixture_through_the_module(tag, mode):
    c = case(tag, mode)
    g, seed, r64 = c["g"], c["seed"], c["r64"]
    got = device_run(tag, mode)
    for k in R.OUTPUTS:
        name = "%s_%s" % (mode, k)
        bar = stage_bar(float(g["dev_" + name]), float(g["max_" + name]))
        check("decoder_%s %s" % (tag, name), got[k], r64[k], bar)
        if name in g:
            check("decoder_%s %s (stored fp32)" % (tag, name), R.sample(got[k].cpu(), seed), torch.from_numpy(g[name]), bar + float(g["dev_" + name]))
    for k in GRADS:
        name = "grad_%s_%s" % (mode, k)
        have, w64, rel = got["grad_" + k], r64["grad_" + k], float(g["rel_" + name])
        assert have is not None and have.shape == w64.shape, k
        bar = max(4.0 * rel, 1e-6)
        check_rel("decoder_%s %s" % (tag, name), have, w64, w64, bar)
        if name in g:
            check_rel("decoder_%s %s (stored fp32)" % (tag, name), R.sample(have.cpu(), seed), torch.from_numpy(g[name]), R.sample(w64, seed), bar + rel)


@pytest.mark.parametrize("tag", FIXTURES)
def test_folded_eval_form_against_the_autograd_form(tag):
    c = case(tag, "eval")
    g = c["g"]
    with torch.no_grad():
        folded = device_run(tag, "eval", backward=False)
    grad_form = device_run(tag, "eval")
    for k in R.OUTPUTS:
        name = "eval_" + k
        bar = stage_bar(float(g["dev_" + name]), float(g["max_" + name]))
        check("decoder_%s %s folded" % (tag, name), folded[k], c["r64"][k], bar)
        check("decoder_%s %s folded - autograd form" % (tag, name), folded[k], grad_form[k], bar)


@pytest.mark.parametrize("mode", R.MODES)
def test_two_runs_give_the_same_bits(mode):
    one, two = device_run("b", mode), device_run("b", mode)
    assert set(one) == set(two) == set(R.OUTPUTS) | {"grad_" + k for k in GRADS}
    for k in one:
        assert same_bits(one[k], two[k]), k


def test_inputs_read_in_place():
    """The four maps as the [B:] halves and channel slices of larger NaN-filled buffers: the bits of contiguous copies, forward and
    backward, and a gradient that is zero outside the slices."""
    tag = "b"
    c = case(tag, "train")
    dense = device_run(tag, "train")
    wide, maps = {}, {}
    for i, (k, v) in enumerate(R.fixture_input(c["seed"], tag).items()):
        B, C, H, W = v.shape
        buf = torch.full((2 * B, C + 3 + i, H, W), float("nan"), device=_dev())
        buf[B:, 1 + i:1 + i + C] = gpu(v)
        wide[k] = buf.requires_grad_(True)
        maps[k] = wide[k][B:, 1 + i:1 + i + C]
        assert not maps[k].is_contiguous()
    sliced = device_run(tag, "train", maps=maps)
    for k in sliced:
        assert same_bits(sliced[k], dense[k]), k
    for i, k in enumerate(R.INPUTS):
        B, C = dense["grad_" + k].shape[:2]
        grad = wide[k].grad
        assert same_bits(grad[B:, 1 + i:1 + i + C], dense["grad_" + k]), k
        assert float(grad[:B].abs().max()) == 0 and float(grad[B:, :1 + i].abs().max()) == 0 and float(grad[B:, 1 + i + C:].abs().max()) == 0


def test_output_written_in_place():
    """Through the C ABI: y as a channel slice of the [B:] half of a sentinel-filled buffer -- the bits of the dense call, nothing else touched."""
    B, Cu, Cs, Cout, h, w, H, W = LAYERS["ragged"]
    a = layer_inputs("ragged")
    up, skip, weight = gpu(a["up"]), gpu(a["skip"]), gpu(a["weight"])
    scale, shift = gpu(a["gamma"]), gpu(a["beta"])
    L = _lib.lib()
    w_l = torch.empty(L.ts_decoder_weight_bytes(Cu + Cs, Cout) // 4, device=_dev())
    _lib.check(L.ts_decoder_weight_layout(_lib.ptr(weight), _lib.ptr(w_l), Cu + Cs, Cout, None), "ts_decoder_weight_layout")
    sentinel = -12345.5
    dense = torch.full((B, Cout, H, W), sentinel, device=_dev())
    buf = torch.full((2 * B, Cout + 5, H, W), sentinel, device=_dev())
    view = buf[B:, 2:2 + Cout]
    for y in (dense, view):
        _lib.check(L.ts_decoder_conv_fwd(_lib.ptr(up), _lib.ptr(skip), _lib.ptr(w_l), _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(y), B, Cu, Cs,
                                         Cout, h, w, H, W, 1, up.stride(0), up.stride(1), skip.stride(0), skip.stride(1), y.stride(0),
                                         y.stride(1), None), "ts_decoder_conv_fwd")
    torch.cuda.synchronize()
    assert same_bits(view, dense) and not bool((dense == sentinel).any())
    rest = buf.clone()
    rest[B:, 2:2 + Cout] = sentinel
    assert bool((rest == sentinel).all())
    r64 = {k: a[k].double() for k in ("up", "skip", "weight", "gamma", "beta")}
    r32 = {k: a[k] for k in r64}
    want = lambda t: torch.nn.functional.silu(R.fused_layer(t["up"], t["skip"], t["weight"]) * t["gamma"].view(1, -1, 1, 1) + t["beta"].view(1, -1, 1, 1))
    w64 = want(r64)
    check("epilogue act(y scale + shift) into a slice", view, w64, stage_bar(float((want(r32).double() - w64).abs().max()), float(w64.abs().max())))


def test_module_routing(monkeypatch):
    """set_conv_backend('torch'), a CPU tensor and a width outside the envelope each reach _reference_forward; fp32 GPU tensors inside the
    envelope under the 'hip' backend do not."""
    calls = []
    real = ts.FeatureDecoder._reference_forward
    monkeypatch.setattr(ts.FeatureDecoder, "_reference_forward", lambda self, *a: calls.append(1) or real(self, *a))
    c = case("a", "eval")
    maps = R.fixture_input(c["seed"], "a")
    on_gpu = [gpu(maps[k]) for k in R.INPUTS]
    m = module_for(c["seed"], False)
    with torch.no_grad():
        m(*on_gpu)
        assert calls == []
        assert layers._CONV_BACKEND["name"] == "hip"
        layers.set_conv_backend("torch")
        try:
            got = m(*on_gpu)
        finally:
            layers.set_conv_backend("hip")
        assert calls == [1]
        for k, t in zip(R.OUTPUTS, got):
            name = "eval_" + k
            check("routing backend 'torch' %s" % k, t, c["r64"][k], stage_bar(float(c["g"]["dev_" + name]), float(c["g"]["max_" + name])))
        m.cpu()(*[maps[k] for k in R.INPUTS])
        assert calls == [1, 1]
        m.to(_dev())
        m.double()(*[t.double() for t in on_gpu])
        assert calls == [1, 1, 1]
        wide = ts.FeatureDecoder(channels=(4, 4, 4, 300, 8), out_channels=(0, 8, 8, 8, 300)).to(_dev()).eval()
        wide(torch.randn(1, 4, 8, 8, device=_dev()), torch.randn(1, 4, 4, 4, device=_dev()), torch.randn(1, 300, 2, 2, device=_dev()),
             torch.randn(1, 8, 1, 1, device=_dev()))
        assert calls == [1, 1, 1, 1]
        other = ts.FeatureDecoder(channels=(4, 4, 4, 4, 8), out_channels=(0, 32, 32, 32, 8), norm="GN").to(_dev()).eval()
        other(torch.randn(1, 4, 8, 8, device=_dev()), torch.randn(1, 4, 4, 4, device=_dev()), torch.randn(1, 4, 2, 2, device=_dev()),
              torch.randn(1, 8, 1, 1, device=_dev()))
        assert calls == [1, 1, 1, 1, 1]


def test_train_forward_updates_the_running_statistics():
    """One train-mode forward moves running_mean / running_var (momentum 0.1, unbiased variance) and num_batches_tracked as the
    restatement's; bars as for a stage, from the restatement's own fp32 and fp64 runs."""
    tag = "b"
    seed = case(tag, "train")["seed"]

    def ref(dt):
        state, maps = R.fixture_state(seed, dt), R.fixture_input(seed, tag, dt)
        with torch.no_grad():
            R.decoder(maps["x4"], maps["x8"], maps["x16"], maps["x32"], state, True, momentum=0.1)
        return state
    s64, s32, before = ref(torch.float64), ref(torch.float32), R.fixture_state(seed)
    m = module_for(seed, True)
    maps = R.fixture_input(seed, tag)
    m(*[gpu(maps[k]) for k in R.INPUTS])                       # with autograd: the training form
    with torch.no_grad():
        m(*[gpu(maps[k]) for k in R.INPUTS])                   # and once more without: the counter and the statistics move again
        R.decoder(*[maps[k].double() for k in R.INPUTS], s64, True, momentum=0.1)
        R.decoder(*[maps[k] for k in R.INPUTS], s32, True, momentum=0.1)
    got = m.state_dict()
    for k in R.KEYS:
        if k.endswith("num_batches_tracked"):
            assert int(got[k]) == 2, k
        elif "running_" in k:
            assert float((s64[k] - before[k].double()).abs().max()) > 1e-3, k           # the statistics did move
            dev = float((s32[k].double() - s64[k]).abs().max())
            check("decoder_%s after two train forwards %s" % (tag, k), got[k], s64[k], stage_bar(dev, float(s64[k].abs().max())))


def test_batchnorm_two_launch_form_equals_the_three_launch_form(monkeypatch):
    """decoder_conv shares conv_bn_act's BatchNorm tail, so TS_BN_FUSED=0 reaches it too: the single-rank two-launch form
    (ts_bn_train_{fwd,bwd}) and the three-launch form (statistics / apply, reduce / apply) take the same partials in the same fixed
    order -- output, five gradients, running statistics and counter identical to the bit (the decoder's counterpart of the test of
    this name in test_conv_autograd_gpu.py)."""
    res = {}
    old = _lib.lib().ts_bn_set_small_elems(0)           # (the layer is small enough for the one-launch form otherwise)
    try:
        for fused in (True, False):
            monkeypatch.setattr(TF, "_BN_FUSED", fused)
            bn = nn.BatchNorm2d(16)
            with torch.no_grad():
                bn.weight.copy_(torch.from_numpy(synth.uniform(7301, "gamma", (16,), 0.5, 1.5)))
                bn.bias.copy_(torch.from_numpy(synth.normal(7301, "beta", (16,), 0.1)))
            bn = bn.to(_dev()).train()
            up = gpu(torch.from_numpy(synth.normal(7301, "up", (2, 8, 5, 7)))).requires_grad_(True)
            skip = gpu(torch.from_numpy(synth.normal(7301, "skip", (2, 8, 9, 13)))).requires_grad_(True)
            weight = gpu(torch.from_numpy(synth.normal(7301, "w", (16, 16, 3, 3), 0.1))).requires_grad_(True)
            out = TF.decoder_conv(up, skip, weight, None, bn, "SiLU")
            out.backward(gpu(torch.from_numpy(synth.normal(7301, "g", (2, 16, 9, 13)))))
            res[fused] = [out.detach(), up.grad, skip.grad, weight.grad, bn.weight.grad, bn.bias.grad, bn.running_mean.clone(),
                          bn.running_var.clone(), bn.num_batches_tracked.clone()]
    finally:
        _lib.lib().ts_bn_set_small_elems(old)
    for a, b in zip(res[True], res[False]):
        assert a is not None and torch.equal(a, b)
    assert int(res[True][-1]) == 1


def test_sync_batchnorm_routing(monkeypatch):
    """A SyncBatchNorm takes the kernels in eval mode and on a single rank; in train mode on more than one rank (a patched
    torch.distributed is enough) the module goes to _reference_forward and functional.decoder_conv refuses."""
    import torch.distributed as dist
    calls = []
    monkeypatch.setattr(ts.FeatureDecoder, "_reference_forward", lambda self, *a: calls.append(1))
    m = ts.FeatureDecoder(channels=(4, 4, 4, 4, 8), out_channels=(0, 8, 8, 8, 8), norm="SyncBN").to(_dev())
    assert isinstance(m.deconv8_4[0].norm, nn.SyncBatchNorm)
    maps = [torch.randn(2, 4, 8, 8, device=_dev()), torch.randn(2, 4, 4, 4, device=_dev()), torch.randn(2, 4, 2, 2, device=_dev()),
            torch.randn(2, 8, 1, 2, device=_dev())]
    m.train()
    assert len(m(*maps)) == 3 and calls == []                  # one rank: the kernels
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    assert TF.bn_exchanges(m.deconv8_4[0].norm)
    m(*maps)
    assert calls == [1]
    conv = m.deconv8_4[0]
    with pytest.raises(RuntimeError, match="SyncBatchNorm"):
        TF.decoder_conv(torch.randn(2, 8, 4, 4, device=_dev()), maps[0], conv.weight, None, conv.norm, "SiLU")
    m.eval()
    with torch.no_grad():
        assert len(m(*maps)) == 3 and calls == [1]             # eval mode: running statistics, nothing to exchange
