"""ConvGRU on the device (temporalstereo_amd.ConvGRU / functional.conv_gru; csrc/conv_gru.hip) against the reference's own runs recorded
in tests/golden/conv_gru_*.npz (tools/gen_golden.py --only-convgru) and against tests/conv_gru_ref.py in fp64 on the CPU.  u = 2^-24.

Bars, none taken from the code under test (the project's convention; the factor 4 is argued in tests/test_raft_corr_gpu.py):
  stages and outputs   |hip - fp64| <= max(4 x dev_stage, 16 u max |stage|), dev_stage = max |fp32 run - fp64 run| of the reference on the
                       CPU: the fixture's, and for the shapes without a fixture (e, f, the routing and range-end cases) the same figure from
                       an fp32 and an fp64 run of conv_gru_ref inside the test.
  gradients            against fp64: relative L2 <= max(4 x rel_grad_key, 1e-6); against the stored fp32 gradients (at the stored
                       positions): that plus rel_grad_key (triangle inequality).
Each case prints error / bar; with TS_CONV_GRU_PARITY_FILE set the line is appended to that file (profiles/conv_gru_parity.txt is made so).
"""
import functools

import numpy as np
import pytest
import torch

import conv_gru_ref as R
from compare import Parity, dev as _dev, gpu, same_bits, stage_bar
import temporalstereo_amd as ts
from temporalstereo_amd import functional as TF
from temporalstereo_amd import layers

pytestmark = pytest.mark.gpu

P = Parity("TS_CONV_GRU_PARITY_FILE", width=52)
check, check_rel = P.check, P.check_rel
#        tag  B  Ch  Cx  H   W
SHAPES = {"a": (2, 12, 5, 9, 37),        # nothing a multiple of a tile; the source seam inside a channel chunk; a batch stride
          "b": (1, 32, 48, 17, 70),      # a row longer than a 64-wide tile; several K chunks
          "c": (2, 64, 64, 6, 20),       # the envelope's maximum: K = 1152, 128 gate rows
          "d": (1, 8, 8, 1, 1),          # only the centre tap is live (forward only)
          "e": (1, 16, 3, 2, 130),       # a very wide two-row plane with a thin x (no fixture)
          "f": (1, 1, 1, 3, 3)}          # one channel on each side (no fixture)
FIXTURES = ("a", "b", "c", "d")
TAGS = tuple(SHAPES)
GRAD_TAGS = ("a", "b", "c", "e", "f")
GRADS = ("h", "x") + R.KEYS


@functools.lru_cache(maxsize=None)
def case(tag):
    """Inputs, the fp64 run of conv_gru_ref and the deviations the bars are made of, computed once and left unchanged."""
    shape = SHAPES[tag]
    backward = tag != "d"
    if tag in FIXTURES:
        g = R.load_fixture(tag)
        assert g["shape"] == shape
        seed = g["seed"]
    else:
        g, seed = None, 4242 + ord(tag)
    r64 = R.run(seed, shape, torch.float64, backward)
    if g is None:
        r32 = R.run(seed, shape, torch.float32, backward)
        dev = {k: float((r32[k].double() - r64[k]).abs().max()) for k in R.STAGES + ("out3",)}
        rel = {k: float((r32["grad_" + k].double() - r64["grad_" + k]).norm() / r64["grad_" + k].norm()) for k in GRADS}
    else:
        dev = {k: float(g["dev_" + k]) for k in R.STAGES + ("out3",)}
        rel = {k: float(g["rel_grad_" + k]) for k in GRADS} if backward else {}
    h, x = R.fixture_input(seed, shape)
    return dict(seed=seed, shape=shape, g=g, r64=r64, dev=dev, rel=rel, h=h, x=x, state=R.fixture_state(seed, shape[1], shape[2]))


def module_for(c, state=None):
    m = ts.ConvGRU(c["shape"][2], c["shape"][1])
    m.load_state_dict(state if state is not None else c["state"], strict=True)
    return m.to(_dev())


def device_chain(c, h=None, x=None, backward=True):
    """three chained steps through ts.ConvGRU and the backward of the seeded cotangent -> out3 and the eight gradients"""
    m = module_for(c)
    h = gpu(c["h"]).requires_grad_(backward) if h is None else h
    x = gpu(c["x"]).requires_grad_(backward) if x is None else x
    o = h
    for _ in range(3):
        o = m(o, x)
    res = dict(out3=o.detach())
    if backward:
        o.backward(gpu(R.fixture_cotangent(c["seed"], o.shape)))
        if h.is_leaf:
            res["grad_h"], res["grad_x"] = h.grad, x.grad
        for k, p in m.named_parameters():
            res["grad_" + k] = p.grad
    return res, h, x


@pytest.mark.parametrize("tag", TAGS)
def test_one_step(tag):
    c = case(tag)
    with torch.no_grad():
        got = TF.conv_gru(gpu(c["h"]), gpu(c["x"]), *[gpu(c["state"][k]) for k in R.KEYS], return_gates=True)
    assert len(got) == 4 and not any(t.requires_grad for t in got)
    for k, t in zip(("out", "z", "r", "q"), got):
        want = c["r64"][k]
        bar = stage_bar(c["dev"][k], float(want.abs().max()))
        check("one step %s %s" % (tag, k), t, want, bar)
        if c["g"] is not None:
            check("one step %s %s (stored fp32)" % (tag, k), R.sample(t.cpu(), c["seed"]), torch.from_numpy(c["g"][k]), bar + c["dev"][k])
    z, r, q = got[1:]
    assert float(z.min()) >= 0 and float(z.max()) <= 1 and float(r.min()) >= 0 and float(r.max()) <= 1 and float(q.abs().max()) <= 1


@pytest.mark.parametrize("tag", TAGS)
def test_three_steps(tag):
    c = case(tag)
    backward = tag in GRAD_TAGS
    res, _, _ = device_chain(c, backward=backward)
    want = c["r64"]["out3"]
    bar = stage_bar(c["dev"]["out3"], float(want.abs().max()))
    check("three steps %s out3" % tag, res["out3"], want, bar)
    if c["g"] is not None:
        check("three steps %s out3 (stored fp32)" % tag, R.sample(res["out3"].cpu(), c["seed"]), torch.from_numpy(c["g"]["out3"]),
              bar + c["dev"]["out3"])
    if not backward:
        return
    for k in GRADS:
        got, w64 = res["grad_" + k], c["r64"]["grad_" + k]
        assert got is not None and got.shape == w64.shape, k
        bar = max(4.0 * c["rel"][k], 1e-6)
        check_rel("three steps %s grad %s" % (tag, k), got, w64, w64, bar)
        if c["g"] is not None:
            check_rel("three steps %s grad %s (stored fp32)" % (tag, k), R.sample(got.cpu(), c["seed"]), torch.from_numpy(c["g"]["grad_" + k]),
                      R.sample(w64, c["seed"]), bar + c["rel"][k])


@pytest.mark.parametrize("tag", ("a", "c"))
def test_two_runs_give_the_same_bits(tag):
    c = case(tag)
    one, _, _ = device_chain(c)
    two, _, _ = device_chain(c)
    assert set(one) == set(two) == {"out3"} | {"grad_" + k for k in GRADS}
    for k in one:
        assert same_bits(one[k], two[k]), k


def test_inputs_read_in_place():
    """last_hidden and x as channel slices of wider tensors (a batch stride that is not C*H*W): the same bits as contiguous copies."""
    c = case("a")
    B, Ch, Cx, H, W = c["shape"]
    wide_h = torch.randn(B, Ch + 5, H, W, device=_dev()).requires_grad_(True)
    wide_x = torch.randn(B, Cx + 3, H, W, device=_dev()).requires_grad_(True)
    with torch.no_grad():
        wide_h[:, 2:2 + Ch] = gpu(c["h"])
        wide_x[:, 1:1 + Cx] = gpu(c["x"])
    hs, xs = wide_h[:, 2:2 + Ch], wide_x[:, 1:1 + Cx]
    assert not hs.is_contiguous() and hs.stride(0) != Ch * H * W
    sliced, _, _ = device_chain(c, hs, xs)
    dense, _, _ = device_chain(c)
    assert same_bits(sliced["out3"], dense["out3"])
    assert same_bits(wide_h.grad[:, 2:2 + Ch], dense["grad_h"]) and same_bits(wide_x.grad[:, 1:1 + Cx], dense["grad_x"])
    assert float(wide_h.grad[:, :2].abs().max()) == 0 and float(wide_h.grad[:, 2 + Ch:].abs().max()) == 0
    for k in R.KEYS:
        assert same_bits(sliced["grad_" + k], dense["grad_" + k]), k


@pytest.mark.parametrize("tag", ("a", "b"))
def test_no_grad_form_has_the_training_forward_bits(tag):
    c = case(tag)
    args = [gpu(c["h"]), gpu(c["x"])] + [gpu(c["state"][k]) for k in R.KEYS]
    with torch.no_grad():
        plain = TF.conv_gru(*args)
    assert not plain.requires_grad
    train = TF.conv_gru(*[a.clone().requires_grad_(True) for a in args])
    assert train.requires_grad and same_bits(plain, train.detach())
    only_x = TF.conv_gru(args[0], args[1].clone().requires_grad_(True), *args[2:])
    only_x.sum().backward()                  # x alone asks for a gradient: dx through ts_conv_gru_grad_sum, nothing else returned
    assert same_bits(plain, only_x.detach())


def test_bits_do_not_depend_on_the_batch_grouping():
    """Eight images of Ch = 64, Cx = 5 on a 31 x 63 plane (the source seam inside a chunk, a ragged last chunk; 32 pixel tiles per
    image, ragged at the right and the bottom) as one call of B = 8, two of B = 4, four of B = 2 and eight of B = 1: hidden, z, r and q
    have the bits of the B = 8 call.  The launch rule (csrc/conv_hw3.hpp launch_rule, at least 256 workgroups) sends the groupings to
        B = 8   gru_conv_kernel<8, true>  gates   gru_conv_kernel<4, false>  candidate
        B = 4   gru_conv_kernel<4, true>          gru_conv_kernel<2, false>
        B = 2   gru_conv_kernel<2, true>          gru_conv_kernel<1, false>
        B = 1   gru_conv_kernel<1, true>          gru_conv_kernel<1, false>
    -- every instantiation there is, where no other shape of this file leaves <1, *>.  Observed in a kernel trace of this test
    (rocprofv3 --kernel-trace, a run of its own): profiles/hw3_grouping_kernel_trace.txt.  The first image's B = 1 result also meets
    the fp64 restatement at the stage bar of the shapes without a fixture."""
    shape, seed = (8, 64, 5, 31, 63), 6405
    h, x = R.fixture_input(seed, shape)
    state = R.fixture_state(seed, shape[1], shape[2])
    hd, xd, params = gpu(h), gpu(x), [gpu(state[k]) for k in R.KEYS]
    names = ("out", "z", "r", "q")

    def grouped(n):
        with torch.no_grad():
            calls = [TF.conv_gru(hd[i:i + n], xd[i:i + n], *params, return_gates=True) for i in range(0, shape[0], n)]
        return dict(zip(names, (torch.cat(t) for t in zip(*calls))))
    whole = grouped(8)
    for n in (4, 2, 1):
        got = grouped(n)
        for k in names:
            assert same_bits(got[k], whole[k]), "B = %d, %s" % (n, k)
    r64 = R.conv_gru(h[:1].double(), x[:1].double(), {k: v.double() for k, v in state.items()})
    r32 = R.conv_gru(h[:1], x[:1], state)
    for k in names:
        dev = float((r32[k].double() - r64[k]).abs().max())
        check("grouping, B = 1, first image %s" % k, got[k][:1], r64[k], stage_bar(dev, float(r64[k].abs().max())))


def _step_with_grads(state, h, x, cot, dtype):
    st = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in state.items()}
    h, x = h.detach().to(dtype).clone().requires_grad_(True), x.detach().to(dtype).clone().requires_grad_(True)
    run = R.conv_gru(h, x, st)
    run["out"].backward(cot.to(dtype))
    return {k: v.detach() for k, v in run.items()}


@pytest.mark.parametrize("bias_scale", (None, 1e30, -1e30))
def test_range_ends(bias_scale):
    """Convolution weights x 1e3 (pre-activations of order 1e3: both gates and the candidate saturate), then the biases x +-1e30."""
    c = case("a")
    state = {k: (v * 1e3 if k.endswith("weight") else (v if bias_scale is None else v * bias_scale)) for k, v in c["state"].items()}
    cot = R.fixture_cotangent(c["seed"], c["h"].shape)
    r64 = _step_with_grads(state, c["h"], c["x"], cot, torch.float64)
    r32 = _step_with_grads(state, c["h"], c["x"], cot, torch.float32)
    args = [gpu(c["h"]).requires_grad_(True), gpu(c["x"]).requires_grad_(True)] + [gpu(state[k]).requires_grad_(True) for k in R.KEYS]
    out, z, r, q = TF.conv_gru(*args, return_gates=True)
    for t in (out, z, r, q):
        assert bool(torch.isfinite(t).all())
    assert float(z.min()) >= 0 and float(z.max()) <= 1 and float(r.min()) >= 0 and float(r.max()) <= 1 and float(q.abs().max()) <= 1
    dev = float((r32["out"].double() - r64["out"]).abs().max())
    check("range ends (bias x %s) hidden" % bias_scale, out.detach(), r64["out"], stage_bar(dev, float(r64["out"].abs().max())))
    out.backward(gpu(cot))
    for a in args:
        assert a.grad is not None and bool(torch.isfinite(a.grad).all())


def _fallback_case(shape, seed):
    r64 = R.run(seed, shape, torch.float64, backward=False)
    r32 = R.run(seed, shape, torch.float32, backward=False)
    h, x = R.fixture_input(seed, shape)
    return dict(seed=seed, shape=shape, h=h, x=x, state=R.fixture_state(seed, shape[1], shape[2]), r64=r64,
                dev=float((r32["out"].double() - r64["out"]).abs().max()))


def test_module_routing(monkeypatch):
    """A cell wider than the kernel path, and any cell under set_conv_backend('torch'), run the reference's op sequence -- never
    functional.conv_gru -- and meet the same bar."""
    def refuse(*a, **k):
        raise AssertionError("functional.conv_gru was called")
    wide = _fallback_case((1, 8, 65, 5, 9), 991)
    inside = _fallback_case(SHAPES["a"], case("a")["seed"])
    calls = []
    real = TF.conv_gru
    monkeypatch.setattr(TF, "conv_gru", lambda *a, **k: calls.append(1) or real(*a, **k))
    with torch.no_grad():
        module_for(inside)(gpu(inside["h"]), gpu(inside["x"]))
    assert calls == [1]                                   # inside the envelope, 'hip' backend: the kernel path
    monkeypatch.setattr(TF, "conv_gru", refuse)
    with torch.no_grad():
        got = module_for(wide)(gpu(wide["h"]), gpu(wide["x"]))
    check("routing ConvGRU(65, 8) fallback", got, wide["r64"]["out"], stage_bar(wide["dev"], float(wide["r64"]["out"].abs().max())))
    assert layers._CONV_BACKEND["name"] == "hip"
    layers.set_conv_backend("torch")
    try:
        with torch.no_grad():
            got = module_for(inside)(gpu(inside["h"]), gpu(inside["x"]))
    finally:
        layers.set_conv_backend("hip")
    check("routing backend 'torch' fallback", got, inside["r64"]["out"], stage_bar(inside["dev"], float(inside["r64"]["out"].abs().max())))
