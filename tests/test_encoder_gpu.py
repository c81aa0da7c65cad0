"""The encoder's large planes on the device (temporalstereo_amd.StemConv / ConvBnAct / FusedInvertedResidual / TemporalStereoBackbone,
functional.conv3x3_bn_act / fused_mbconv_eval; csrc/fused_mbconv.hip) against the reference's own runs recorded in
tests/golden/encoder_*.npz (tools/gen_golden.py --only-encoder) and against tests/encoder_ref.py and plain torch in fp64 on the CPU.
u = 2^-24.

Bars, those of tests/test_mbconv_gpu.py unchanged; none is taken from the code under test:
  stages and outputs   |hip - fp64| <= max(4 x dev_stage, 16 u max |stage|), dev_stage = max |fp32 run - fp64 run| of the reference on the
                       CPU: the fixture's, and for the shapes without a fixture (the single entries, the range case, the running
                       statistics) the same figure from an fp32 and an fp64 run of the same torch statements inside the test.
  gradients            against fp64: relative L2 <= max(4 x rel_grad_key, 1e-6).
Each case prints error / bar; with TS_ENCODER_PARITY_FILE set the line is appended to that file (profiles/encoder_parity.txt is made so).
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import encoder_ref as R
import synth
from compare import Parity, dev as _dev, gpu, same_bits, stage_bar
import temporalstereo_amd as ts
from temporalstereo_amd import _lib
from temporalstereo_amd import functional as TF
from temporalstereo_amd import layers

pytestmark = pytest.mark.gpu

P = Parity("TS_ENCODER_PARITY_FILE", width=72)
check, check_rel, against_fp64 = P.check, P.check_rel, P.against_fp64
MP = R.MEMORY_PERCENT
PLANES = ((1, 1), (1, 5), (5, 1), (2, 2), (5, 7), (6, 8), (3, 70), (40, 3), (9, 66))
WIDTHS = ((3, 8), (12, 24), (24, 40), (48, 192))          # (Cin, Cout): 40 is no multiple of 16, 192 is more than one row group


def t32(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float32))


# ------------------------------------------------------------------------------------------------------------------ the modules
@functools.lru_cache(maxsize=None)
def case(tag, mode):
    g = R.load_fixture(tag)
    with torch.enable_grad():
        return dict(g=g, seed=g["seed"], r64=R.run(g["seed"], tag, torch.float64, mode == "train"))


def own_net(tag, seed, training, scale=1.0):
    c = R.CASES[tag]
    if c["kind"] == "backbone":
        net = ts.TemporalStereoBackbone(arch=R.MINI, memory_percent=MP)
    else:
        net = nn.Sequential(nn.Sequential(*[ts.FusedInvertedResidual(cin, cout, stride=s, mid_chs=cmid) for cin, cmid, cout, s in c["members"]]))
    state = R.fixture_state(seed, tag)
    if scale != 1.0:
        state = {k: v * scale if v.dim() == 4 else v for k, v in state.items()}
    net.load_state_dict(state, strict=True)
    return net.to(_dev()).train(training)


def backbone_by_hand(net, l_img, r_img, memories, want_route=None):
    """TemporalStereoBackbone._forward's statements, keeping what lies in front of the decoder."""
    stem, decoder = net._parts
    x = torch.cat([l_img, r_img], 0)
    if want_route is not None:
        assert stem._route(x) == want_route
    res = {}
    x = res["stem"] = stem(x)
    if want_route is not None:
        assert net.block0[0][0]._route(x) == want_route
    x = res["block0"] = net.block0(x)
    idx, out = 0, []
    for i in range(1, 5):
        if want_route is not None and i < 3:
            assert getattr(net, "block%d" % i)[0][0]._route(x) == want_route
        x, new, idx = ts.block_forward(getattr(net, "block%d" % i), x, net.memory_percent, memories, idx)
        out.extend(new)
        res["block%d" % i] = x
    for k, v in zip(R.OUTS, decoder(res["block1"], res["block2"], res["block3"], res["block4"])):
        res[k] = v
    return res, out


def device_run(tag, mode, stages=False, net=None):
    """The package's modules on the fixture's inputs -> dict(f<frame>_<stage | out>, grad_*); stages: the walk by hand, every stage."""
    c = case(tag, mode)
    seed, training, kind = c["seed"], mode == "train", R.CASES[tag]["kind"]
    net = own_net(tag, seed, training) if net is None else net
    ins = [gpu(t).requires_grad_(training) for t in R.fixture_inputs(seed, tag)]
    route = "train" if training else "kernels"
    res, outs = {}, []
    if kind == "backbone":
        info, memories = {}, []
        for f in range(R.CASES[tag]["frames"]):
            if stages:
                r, memories = backbone_by_hand(net, ins[2 * f], ins[2 * f + 1], memories, route)
                for k, v in r.items():
                    res["f%d_%s" % (f, k)] = v.detach()
            else:
                l_fms, r_fms, info = net(ins[2 * f], ins[2 * f + 1], info)
                for k, l, r in zip(R.OUTS, l_fms, r_fms):
                    outs.append(torch.cat([l, r], 0))
                    res["f%d_%s" % (f, k)] = outs[-1].detach()
                memories = info["memories"]
            assert [tuple(m.shape) for m in memories] == [(4, 6, 4, 6), (4, 8, 2, 3)] and all(m._base is not None for m in memories)
    elif stages:
        x = ins[0]
        for i, blk in enumerate(net[0]):
            assert blk._route(x) == "kernels"
            x, st = blk._kernel_forward(x, return_stages=True)
            res["f0_b%d_mid" % i], res["f0_b%d_out" % i] = st["mid"], x
        res["f0_out"] = x
    else:
        assert net[0][0]._route(ins[0]) == route
        if kind == "stage":
            out, memories, idx = ts.block_forward(net, ins[0], MP, None, 0)
            assert memories == [] and idx == 0
        else:
            out = net[0][0](ins[0])
        outs.append(out)
        res["f0_out"] = out.detach()
    if training:
        torch.autograd.backward(outs, [gpu(t) for t in R.fixture_cotangents(seed, tag)])
        for name, x in zip(R.input_names(tag), ins):
            res["grad_" + name] = x.grad
        for k, p in net.named_parameters():
            res["grad_" + k] = p.grad
    return res


def compare_forward(tag, mode, got, label=""):
    c = case(tag, mode)
    g, seed, r64 = c["g"], c["seed"], c["r64"]
    for k in [k for k in got if not k.startswith("grad_")]:
        name = "%s_%s" % (mode, k)
        bar = stage_bar(float(g["dev_" + name]), float(g["max_" + name]))
        check("encoder_%s %s%s" % (tag, name, label), got[k], r64[k], bar)
        if name in g:
            check("encoder_%s %s%s (stored fp32)" % (tag, name, label), R.sample(got[k].cpu(), seed), torch.from_numpy(g[name]), bar + float(g["dev_" + name]))


def compare_grads(tag, got, label=""):
    c = case(tag, "train")
    g, r64 = c["g"], c["r64"]
    grads = [k for k in r64 if k.startswith("grad_")]
    assert set(grads) == {k for k in got if k.startswith("grad_")}
    for k in grads:
        name = "grad_train_" + k[5:]
        have, w64 = got[k], r64[k]
        assert have is not None and have.shape == w64.shape, k
        check_rel("encoder_%s %s%s" % (tag, name, label), have, w64, w64, max(4.0 * float(g["rel_" + name]), 1e-6))


@pytest.mark.parametrize("tag", R.TAGS)
def test_fixture_in_eval_mode_every_stage(tag):
    with torch.no_grad():
        got = device_run(tag, "eval", stages=True)
    assert set(got) == {k for k in case(tag, "eval")["r64"] if not k.startswith("grad_")}
    compare_forward(tag, "eval", got)


@pytest.mark.parametrize("tag", R.TAGS)
def test_fixture_in_train_mode(tag):
    got = device_run(tag, "train")
    compare_forward(tag, "train", got)
    compare_grads(tag, got)


@pytest.mark.parametrize("tag", R.TAGS)
def test_train_forwards_update_the_running_statistics(tag):
    """Two train-mode passes over the fixture's frames move running_mean / running_var (momentum 0.1, unbiased variance) and
    num_batches_tracked as the restatement's; bars as for a stage, from the restatement's own fp32 and fp64 runs."""
    seed, frames = case(tag, "train")["seed"], R.CASES[tag]["frames"]

    def ref(dt):
        state = R.fixture_state(seed, tag, dt)
        with torch.no_grad():
            for _ in range(2):
                R.forward(tag, state, R.fixture_inputs(seed, tag, dt), True, momentum=0.1)
        return state
    s64, s32, before = ref(torch.float64), ref(torch.float32), R.fixture_state(seed, tag)
    net = own_net(tag, seed, True)
    ins = [gpu(t) for t in R.fixture_inputs(seed, tag)]

    def once():
        if R.CASES[tag]["kind"] == "backbone":
            info = {}
            for f in range(frames):
                _, _, info = net(ins[2 * f], ins[2 * f + 1], info)
        else:
            ts.block_forward(net, ins[0], MP, None, 0)
    once()                                                      # with autograd
    with torch.no_grad():
        once()                                                  # and once more without
    got = net.state_dict()
    for k, _ in R.key_shapes(tag):
        if k.endswith("num_batches_tracked"):
            assert int(got[k]) == 2 * frames, k
        elif "running_" in k:
            assert float((s64[k] - before[k].double()).abs().max()) > 1e-3, k
            check("encoder_%s after two train passes %s" % (tag, k), got[k], s64[k],
                  stage_bar(float((s32[k].double() - s64[k]).abs().max()), float(s64[k].abs().max())))


@pytest.mark.parametrize("mode", R.MODES)
def test_two_runs_give_the_same_bits(mode, monkeypatch):
    # train mode: the 1x1 and stride-2 convolutions and their BatchNorms are the framework's there; it is asked for its deterministic algorithms
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)

    def once():
        if mode == "eval":
            with torch.no_grad():
                return device_run("d", mode, stages=True)
        return device_run("c", mode)
    one, two = once(), once()
    assert set(one) == set(two) and len(one) >= 10
    for k in one:
        assert same_bits(one[k], two[k]), k


def test_batch_slices_equal_single_image_calls():
    """B = 2 through the eval form equals two B = 1 calls bit for bit, for the strided and the residual block: no sum depends on the batch
    or on the grid it makes."""
    seed = case("c", "eval")["seed"]
    net = own_net("c", seed, False)
    x = gpu(R.fixture_inputs(seed, "c")[0])
    with torch.no_grad():
        for blk in net[0]:
            both, st = blk._kernel_forward(x, return_stages=True)
            for b in range(2):
                one, st1 = blk._kernel_forward(x[b:b + 1], return_stages=True)
                assert same_bits(one, both[b:b + 1]) and same_bits(st1["mid"], st["mid"][b:b + 1]), b
            x = both


def test_weights_scaled_by_1e3():
    """Every convolution weight times 1e3: the pre-activations reach the far ends of SiLU; everything stays finite and within the bars of
    the restatement's own fp32 run."""
    tag = "a"
    seed = case(tag, "eval")["seed"]
    x = R.fixture_inputs(seed, tag)[0]

    def ref(dt):
        state = {k: (v * 1e3 if v.dim() == 4 else v) for k, v in R.fixture_state(seed, tag, dt).items()}
        out, mid = R.edge(x.to(dt), state, "0.0.", 1, True, False)
        return dict(mid=mid, out=out)
    r64, r32 = ref(torch.float64), ref(torch.float32)
    blk = own_net(tag, seed, False, scale=1e3)[0][0]
    with torch.no_grad():
        out, got = blk._kernel_forward(gpu(x), return_stages=True)
    got["out"] = out
    assert float(r64["mid"].abs().max()) > 1e3
    for k in ("mid", "out"):
        assert bool(torch.isfinite(got[k]).all()), k
        check("encoder_a, weights x 1e3, %s" % k, got[k], r64[k], stage_bar(float((r32[k].double() - r64[k]).abs().max()), float(r64[k].abs().max())))


# ------------------------------------------------------------------------------------------------------------------ the entries alone
def laid3(weight, stride):
    """ts_conv3x3_s_weight_layout of a [Cout, Cin, 3, 3] weight on the device"""
    Cout, Cin = weight.shape[:2]
    w_l = torch.empty(_lib.lib().ts_conv3x3_s_weight_bytes(Cin, Cout, stride) // 4, device=_dev())
    _lib.check(_lib.lib().ts_conv3x3_s_weight_layout(_lib.ptr(weight), _lib.ptr(w_l), Cin, Cout, stride, None), "ts_conv3x3_s_weight_layout")
    return w_l


def laid1(weight):
    """ts_mbconv_weight_layout of a [Cout, Cin] weight on the device"""
    Cout, Cin = weight.shape
    w_l = torch.empty(_lib.lib().ts_mbconv_weight_bytes(Cin, Cout) // 4, device=_dev())
    _lib.check(_lib.lib().ts_mbconv_weight_layout(_lib.ptr(weight), _lib.ptr(w_l), Cin, Cout, None), "ts_mbconv_weight_layout")
    return w_l


def conv3_call(x, w_l, scale, shift, res, y, stride, act, Cout):
    B, Cin, H, W = x.shape
    rb, rc = (res.stride(0), res.stride(1)) if res is not None else (0, 0)
    rc_ = _lib.lib().ts_conv3x3_s_fwd(_lib.ptr(x), _lib.ptr(w_l), _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(res), _lib.ptr(y), B, Cin, Cout, H, W,
                                      stride, act, x.stride(0), x.stride(1), rb, rc, y.stride(0), y.stride(1), None)
    _lib.check(rc_, "ts_conv3x3_s_fwd")


def conv3_want(stride, act, affine, residual):
    def want(x, w, scale, shift, res):
        y = F.conv2d(x, w, None, stride, 1)
        if affine:
            y = y * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
        if act:
            y = F.silu(y)
        return y + res if residual else y
    return want


def conv3_inputs(seed, B, Cin, Cout, plane, stride):
    H, W = plane
    Ho, Wo = (H + stride - 1) // stride, (W + stride - 1) // stride
    return (t32(synth.normal(seed, "x", (B, Cin, H, W))), t32(synth.normal(seed, "w", (Cout, Cin, 3, 3)).astype(np.float64) * (2.0 / np.sqrt(9.0 * Cin))),
            t32(synth.uniform(seed, "s", (Cout,), 0.5, 1.5)), t32(synth.normal(seed, "b", (Cout,), 0.1)), t32(synth.normal(seed, "r", (B, Cout, Ho, Wo))))


@pytest.mark.parametrize("plane", PLANES)
@pytest.mark.parametrize("stride", (1, 2))
def test_conv3x3_entry(stride, plane):
    """Every plane (one pixel; one row; one column; both parities; more than one 32-column tile, ragged: at stride 2 the output planes 1x1,
    3x4, 2x35 and 5x33 among them) at the four width pairs; the options rotate with the pair: SiLU, scale / shift, and at stride 1 the
    residual, each present in two pairs and absent in two."""
    B = 2
    for i, (Cin, Cout) in enumerate(WIDTHS):
        act, affine, residual = int(i % 2 == 0), i in (0, 3), stride == 1 and i in (1, 3)
        seed = 8100 + 1000 * stride + 100 * plane[0] + plane[1] + 7 * i
        x, w, scale, shift, res = conv3_inputs(seed, B, Cin, Cout, plane, stride)
        y = torch.full(res.shape, float("nan"), device=_dev())
        held = [gpu(x), laid3(gpu(w), stride), gpu(scale) if affine else None, gpu(shift) if affine else None, gpu(res) if residual else None]
        conv3_call(*held, y, stride, act, Cout)
        against_fp64("conv3x3 s%d %dx%d %d -> %d act %d affine %d residual %d" % (stride, plane[0], plane[1], Cin, Cout, act, affine, residual),
                     y, conv3_want(stride, act, affine, residual), (x, w, scale, shift, res))


@pytest.mark.parametrize("stride", (1, 2))
def test_conv3x3_cross_of_widths_and_options(stride):
    """Every Cin in {3, 12, 24, 48} with every Cout in {8, 24, 40, 192} on the 5 x 7 plane, each with every combination of SiLU, scale /
    shift and (at stride 1) the residual -- the residual together with SiLU is what tells the ConvBnAct order, residual after the
    activation, from the other."""
    B, plane = 2, (5, 7)
    for Cin in (3, 12, 24, 48):
        for Cout in (8, 24, 40, 192):
            seed = 8200 + 1000 * stride + 10 * Cin + Cout
            x, w, scale, shift, res = conv3_inputs(seed, B, Cin, Cout, plane, stride)
            xd, w_l, sd, bd, rd = gpu(x), laid3(gpu(w), stride), gpu(scale), gpu(shift), gpu(res)
            for act in (0, 1):
                for affine in (False, True):
                    for residual in ((False, True) if stride == 1 else (False,)):
                        y = torch.full(res.shape, float("nan"), device=_dev())
                        conv3_call(xd, w_l, sd if affine else None, bd if affine else None, rd if residual else None, y, stride, act, Cout)
                        against_fp64("conv3x3 s%d 5x7 cross %d -> %d act %d affine %d residual %d" % (stride, Cin, Cout, act, affine, residual),
                                     y, conv3_want(stride, act, affine, residual), (x, w, scale, shift, res))


@pytest.mark.parametrize("stride", (1, 2))
def test_conv3x3_operands_read_in_place_and_output_written_into_a_slice(stride):
    """x a channel slice of a NaN-filled wider tensor, the residual a batch slice, y a channel slice of a sentinel-filled tensor: the bits of
    the dense call, the guards untouched."""
    B, Cin, Cout, plane = 2, 12, 40, (9, 13)
    x, w, scale, shift, res = conv3_inputs(8300 + stride, B, Cin, Cout, plane, stride)
    residual = stride == 1
    xd, w_l, sd, bd, rd = gpu(x), laid3(gpu(w), stride), gpu(scale), gpu(shift), gpu(res)
    dense = torch.full(res.shape, float("nan"), device=_dev())
    conv3_call(xd, w_l, sd, bd, rd if residual else None, dense, stride, 1, Cout)
    wide_x = torch.full((B, Cin + 5) + plane, float("nan"), device=_dev())
    wide_x[:, 2:2 + Cin] = xd
    wide_r = torch.full((2 * B,) + tuple(res.shape[1:]), float("nan"), device=_dev())
    wide_r[B:] = rd
    sentinel = -12345.5
    wide_y = torch.full((B, Cout + 3) + tuple(res.shape[2:]), sentinel, device=_dev())
    view = wide_y[:, 1:1 + Cout]
    before = wide_x.clone()
    conv3_call(wide_x[:, 2:2 + Cin], w_l, sd, bd, wide_r[B:] if residual else None, view, stride, 1, Cout)
    torch.cuda.synchronize()
    assert same_bits(view, dense) and not bool((dense == sentinel).any()) and bool(torch.isfinite(dense).all())
    assert bool((wide_y[:, :1] == sentinel).all()) and bool((wide_y[:, 1 + Cout:] == sentinel).all())
    assert same_bits(wide_x.nan_to_num(7.0), before.nan_to_num(7.0))
    against_fp64("conv3x3 s%d, strided operands" % stride, view, conv3_want(stride, 1, True, residual), (x, w, scale, shift, res))
    # the functional entry takes the same views
    with torch.no_grad():
        out = TF.conv3x3_bn_act(wide_x[:, 2:2 + Cin], gpu(w), (sd, bd), stride, "SiLU", residual=wide_r[B:] if residual else None)
    assert same_bits(out, dense)
    if residual:                                                        # y may be the residual's own elements: an update in place
        own = rd.clone()
        conv3_call(xd, w_l, sd, bd, own, own, stride, 1, Cout)
        assert same_bits(own, dense)
        shifted = torch.zeros(own.numel() + 1, device=_dev())
        rc = _lib.lib().ts_conv3x3_s_fwd(_lib.ptr(xd), _lib.ptr(w_l), None, None, _lib.ptr(shifted[1:]), _lib.ptr(shifted), B, Cin, Cout, plane[0],
                                         plane[1], 1, 0, xd.stride(0), xd.stride(1), own.stride(0), own.stride(1), own.stride(0), own.stride(1), None)
        assert rc == -2 and b"residual" in _lib.lib().ts_last_error_string()          # a shifted overlap is refused


@pytest.mark.parametrize("Cmid", (40, 96, 256))
def test_fused_project_entry(Cmid):
    """B = 2, Cout = 24 on 9 x 13 (two pixel tiles, the second ragged); Cmid = 40 has a ragged second chunk, 256 is eight full chunks; the
    residual and the output are channel slices of wider tensors, then the residual, scale and shift absent."""
    B, C, H, W = 2, 24, 9, 13
    seed = 8400 + Cmid
    x = t32(synth.normal(seed, "x", (B, Cmid, H, W)))
    w = t32(synth.normal(seed, "w", (C, Cmid)).astype(np.float64) * (2.0 / np.sqrt(Cmid)))
    scale, shift = t32(synth.uniform(seed, "s", (C,), 0.5, 1.5)), t32(synth.normal(seed, "b", (C,), 0.1))
    res = t32(synth.normal(seed, "r", (B, C, H, W)))
    wide_r = torch.full((B, C + 7, H, W), float("nan"), device=_dev())
    wide_r[:, 4:4 + C] = gpu(res)
    rv = wide_r[:, 4:4 + C]
    w_l, xd, sd, bd = laid1(gpu(w)), gpu(x), gpu(scale), gpu(shift)
    for full in (True, False):
        wide_y = torch.full((B, C + 3, H, W), -7.25, device=_dev())
        yv = wide_y[:, 1:1 + C]
        rc = _lib.lib().ts_fused_project_fwd(_lib.ptr(xd), _lib.ptr(w_l), _lib.ptr(sd) if full else None, _lib.ptr(bd) if full else None,
                                             _lib.ptr(rv) if full else None, _lib.ptr(yv), B, Cmid, C, H, W, Cmid * H * W, H * W,
                                             rv.stride(0) if full else 0, rv.stride(1) if full else 0, yv.stride(0), yv.stride(1), None)
        _lib.check(rc, "ts_fused_project_fwd")

        def want(x, w, scale, shift, res):
            y = F.conv2d(x, w[:, :, None, None])
            return y * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1) + res if full else y
        against_fp64("fused project Cmid %d, residual / affine %s" % (Cmid, full), yv, want, (x, w, scale, shift, res))
        assert bool((wide_y[:, :1] == -7.25).all()) and bool((wide_y[:, 1 + C:] == -7.25).all())


@pytest.mark.parametrize("stride", (1, 2))
def test_conv3x3_bits_do_not_depend_on_the_batch_grouping(stride):
    """conv3x3_kernel at every MT.  44 core channels (six chunks: one flush of the blocked sums is crossed, the last chunk ragged; at
    stride 2 they are the phases of 11 input channels on 47 x 47, odd on both axes), 130 output rows (a ragged last row group at every
    MT), output plane 24 x 24 (twelve pixel tiles an image).  The launch rule (csrc/conv_hw3.hpp launch_rule, at least 512 workgroups)
    sends the first n images to
        n = 22  <8> (264 tiles x 2 row groups)    n = 16  <4> (192 x 3)    n = 10  <2> (120 x 5)    n = 4  <1> (48 x 9)
    Every grouping has the bits of the n = 22 call; the n = 4 result also meets the fp64 statement at the stage bar."""
    B, rows = 22, 130
    Cin, plane = (44, (24, 24)) if stride == 1 else (11, (47, 47))
    x, w, scale, shift, res = conv3_inputs(8500 + stride, B, Cin, rows, plane, stride)
    residual = stride == 1
    xd, w_l, sd, bd, rd = gpu(x), laid3(gpu(w), stride), gpu(scale), gpu(shift), gpu(res)

    def call(n):
        y = torch.full((n,) + tuple(res.shape[1:]), float("nan"), device=_dev())
        conv3_call(xd[:n], w_l, sd, bd, rd[:n] if residual else None, y, stride, 1, rows)
        return y
    whole = call(B)
    assert tuple(whole.shape[2:]) == (24, 24)
    for n in (16, 10, 4):
        got = call(n)
        assert same_bits(got, whole[:n]), "first %d images" % n
    against_fp64("grouping, conv3x3 s%d, first 4 images" % stride, got, conv3_want(stride, 1, True, residual), (x[:4], w, scale, shift, res[:4]))


def test_fused_project_bits_do_not_depend_on_the_batch_grouping():
    """fused_project_kernel at every MT, the shapes of tests/test_mbconv_gpu.py's pointwise case: 300 input channels, 130 output rows, a
    24 x 24 plane; n = 32 <8>, 20 <4>, 12 <2>, 4 <1>."""
    B, Cin, rows, H, W = 32, 300, 130, 24, 24
    seed = 8600
    scale, shift = t32(synth.uniform(seed, "s", (rows,), 0.5, 1.5)), t32(synth.normal(seed, "b", (rows,), 0.1))
    w = t32(synth.normal(seed, "w", (rows, Cin)).astype(np.float64) * (2.0 / np.sqrt(Cin)))
    x, res = t32(synth.normal(seed, "x", (B, Cin, H, W))), t32(synth.normal(seed, "r", (B, rows, H, W)))
    sd, bd, w_l, xd, rd = gpu(scale), gpu(shift), laid1(gpu(w)), gpu(x), gpu(res)
    N = H * W

    def call(n):
        y = torch.full((n, rows, H, W), float("nan"), device=_dev())
        _lib.check(_lib.lib().ts_fused_project_fwd(_lib.ptr(xd), _lib.ptr(w_l), _lib.ptr(sd), _lib.ptr(bd), _lib.ptr(rd), _lib.ptr(y), n, Cin, rows,
                                                   H, W, Cin * N, N, rows * N, N, rows * N, N, None), "ts_fused_project_fwd")
        return y
    whole = call(B)
    for n in (20, 12, 4):
        got = call(n)
        assert same_bits(got, whole[:n]), "first %d images" % n
    against_fp64("grouping, fused project, first 4 images", got,
                 lambda x, w, scale, shift, res: F.conv2d(x, w[:, :, None, None]) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1) + res,
                 (x[:4], w, scale, shift, res[:4]))


def test_entry_refusals():
    """Envelope, NULL pointer and overlap return the error codes; nothing is launched."""
    L = _lib.lib()
    x, y = torch.zeros(1, 8, 4, 4, device=_dev()), torch.full((1, 8, 4, 4), 3.0, device=_dev())
    w_l = torch.zeros(L.ts_conv3x3_s_weight_bytes(8, 8, 1) // 4, device=_dev())
    N = 16
    args = lambda x_=x, y_=y, w_=w_l, Cin=8, stride=1: (_lib.ptr(x_), _lib.ptr(w_), None, None, None, _lib.ptr(y_), 1, Cin, 8, 4, 4, stride, 0,
                                                        Cin * N, N, 0, 0, 8 * N, N, None)
    assert L.ts_conv3x3_s_fwd(*args(Cin=513)) == -3 and L.ts_conv3x3_s_fwd(*args(Cin=129, stride=2)) == -3
    assert L.ts_conv3x3_s_fwd(*args(x_=None)) == -1 and L.ts_conv3x3_s_fwd(*args(y_=None)) == -1
    assert L.ts_conv3x3_s_fwd(*args(y_=x)) == -2 and b"overlaps" in L.ts_last_error_string()
    a = list(args())
    a[14] = N - 1                                              # the channel stride of x shorter than a plane
    assert L.ts_conv3x3_s_fwd(*a) == -2 and b"overlap" in L.ts_last_error_string()
    pa = lambda x_=x, y_=y, Cmid=8: (_lib.ptr(x_), _lib.ptr(w_l), None, None, None, _lib.ptr(y_), 1, Cmid, 8, 4, 4, Cmid * N, N, 0, 0, 8 * N, N, None)
    assert L.ts_fused_project_fwd(*pa(Cmid=2049)) == -3 and L.ts_fused_project_fwd(*pa(x_=None)) == -1 and L.ts_fused_project_fwd(*pa(y_=x)) == -2
    torch.cuda.synchronize()
    assert bool((y == 3.0).all())
    with pytest.raises(RuntimeError, match="outside the kernel path"):
        TF.conv3x3_bn_act(torch.zeros(1, 129, 4, 4, device=_dev()), torch.zeros(8, 129, 3, 3, device=_dev()), None, 2, None)
    with pytest.raises(ValueError, match="stride 1 only"):
        TF.conv3x3_bn_act(x, torch.zeros(8, 8, 3, 3, device=_dev()), None, 2, None, residual=torch.zeros(1, 8, 2, 2, device=_dev()))
    with pytest.raises(RuntimeError, match="GPU only"):
        TF.conv3x3_bn_act(x.cpu(), torch.zeros(8, 8, 3, 3), None, 1, None)


# ------------------------------------------------------------------------------------------------------------------ routing, launches
def test_module_routing(monkeypatch):
    """set_conv_backend('torch'), fp64, CPU tensors, stochastic depth in train mode, a real squeeze-excite and a strided conv_pwl reach
    _reference_forward; train mode (or a gradient asked for) reaches _train_forward; eval mode on fp32 GPU tensors under the 'hip' backend
    reaches the kernels."""
    calls = []
    M = ts.FusedInvertedResidual
    for name in ("_reference_forward", "_train_forward", "_kernel_forward"):
        real = getattr(M, name)
        monkeypatch.setattr(M, name, lambda self, *a, real=real, name=name, **k: calls.append(name) or real(self, *a, **k))
    tag = "a"
    c = case(tag, "eval")
    g, x = c["g"], R.fixture_inputs(c["seed"], tag)[0]
    xd = gpu(x)
    m = own_net(tag, c["seed"], False)[0][0]
    bar = stage_bar(float(g["dev_eval_f0_out"]), float(g["max_eval_f0_out"]))
    with torch.no_grad():
        m(xd)
        assert calls == ["_kernel_forward"]
        assert layers._CONV_BACKEND["name"] == "hip"
        layers.set_conv_backend("torch")
        try:
            got = m(xd)
        finally:
            layers.set_conv_backend("hip")
        assert calls[1:] == ["_reference_forward"]
        check("routing backend 'torch' out", got, c["r64"]["f0_out"], bar)
        m.cpu()(x)
        m.to(_dev())
        m.double()(xd.double())
        m.float()
        assert calls[2:] == ["_reference_forward"] * 2
        wide = M(516, 8, mid_chs=8).to(_dev()).eval()
        wide(torch.randn(1, 516, 3, 3, device=_dev()))
        assert calls[4:] == ["_reference_forward"]
    got = m(xd.clone().requires_grad_(True))                           # eval mode, a gradient asked for
    assert calls[5:] == ["_train_forward"] and got.requires_grad
    check("routing eval mode with a gradient, out", got.detach(), c["r64"]["f0_out"], bar)
    m.train()
    with torch.no_grad():
        m(xd)
    assert calls[6:] == ["_train_forward"]
    m.drop_path_rate = 0.2                                             # stochastic depth in train mode
    with torch.no_grad():
        m(xd)
    assert calls[7:] == ["_reference_forward"]
    m.eval()
    with torch.no_grad():
        m(xd)                                                          # ... and none in eval mode
    assert calls[8:] == ["_kernel_forward"]
    m.drop_path_rate = 0.0
    m.bn2.train()                                                      # one BatchNorm in train mode is train mode
    with torch.no_grad():
        m(xd)
    assert calls[9:] == ["_train_forward"] and len(calls) == 10
    m.eval()

    class RealSE(nn.Module):
        def forward(self, t):
            return t * 0.5
    for change in (lambda b: setattr(b, "se", RealSE()), lambda b: setattr(b, "conv_pwl", nn.Conv2d(96, 24, 1, 2, bias=False))):
        theirs = R.StandInEdge(24, 96, 24, 1)
        theirs.load_state_dict(m.state_dict(), strict=True)
        change(theirs)
        theirs.has_residual = isinstance(theirs.se, RealSE)
        theirs = theirs.to(_dev()).eval()
        other = M.from_block(theirs)
        del calls[:]
        with torch.no_grad():
            assert not other._recognised and torch.equal(other(xd), theirs(xd))
        assert calls == ["_reference_forward"]
    # the two one-launch modules decide the same way
    for blk, inp in ((ts.ConvBnAct(24, 24, skip=True), xd), (ts.StemConv(24, 8), xd)):
        blk = blk.to(_dev()).eval()
        with torch.no_grad():
            assert blk._route(inp) == "kernels" and blk._route(inp.cpu()) == "reference" and blk._route(inp.double()) == "reference"
        assert blk._route(inp) == "train"                               # the parameters ask for a gradient
        blk.train()
        with torch.no_grad():
            assert blk._route(inp) == "train"


def test_one_launch_modules_against_fp64():
    """ConvBnAct (with its skip) and StemConv (stride 2, odd plane) in eval mode, and their train route with gradients, against the same
    torch statements in fp64."""
    for name, make, shape in (("ConvBnAct", lambda: ts.ConvBnAct(24, 24, skip=True), (2, 24, 9, 13)), ("StemConv", lambda: ts.StemConv(3, 24), (2, 3, 17, 31))):
        torch.manual_seed(11)
        ref = make()
        with torch.no_grad():
            for bn in (ref.bn1,):
                bn.running_mean.normal_(0, 0.1)
                bn.running_var.uniform_(0.5, 1.5)
                bn.weight.uniform_(0.5, 1.5)
                bn.bias.normal_(0, 0.1)
        x = torch.randn(shape)
        mod = make()
        mod.load_state_dict(ref.state_dict())
        mod = mod.to(_dev())
        for training in (False, True):
            def run(dt):
                r = make()
                r.load_state_dict(ref.state_dict())
                r = r.to(dt).train(training)
                xx = x.clone().to(dt).requires_grad_(True)
                y = r._reference_forward(xx)
                y.backward(R.cotangent(8700, name, y.shape, dt))
                return [y.detach(), xx.grad] + [p.grad for p in r.parameters()]
            r64, r32 = run(torch.float64), run(torch.float32)
            mod.train(training)
            xd = gpu(x).requires_grad_(True)
            if not training:
                with torch.no_grad():
                    assert mod._route(xd) == "kernels"
                    y = mod(xd)
                check("%s eval out" % name, y, r64[0], stage_bar(float((r32[0].double() - r64[0]).abs().max()), float(r64[0].abs().max())))
                continue
            assert mod._route(xd) == "train"
            mod.zero_grad()
            y = mod(xd)
            y.backward(gpu(R.cotangent(8700, name, y.shape)))
            check("%s train out" % name, y.detach(), r64[0], stage_bar(float((r32[0].double() - r64[0]).abs().max()), float(r64[0].abs().max())))
            for what, have, w64, w32 in zip(["x"] + [k for k, _ in mod.named_parameters()], [xd.grad] + [p.grad for p in mod.parameters()], r64[1:], r32[1:]):
                check_rel("%s train grad %s" % (name, what), have, w64, w64, max(4.0 * float((w32.double() - w64).norm() / w64.norm()), 1e-6))


def test_eval_launch_counts():
    """Inside WeightLayouts and BNFolds contexts an eval fused block issues exactly two launches and a ConvBnAct or the stem one (the first
    call lays the weights out and folds the BatchNorms); a bare call adds its weight layouts and folds."""
    c = case("a", "eval")
    m = own_net("a", c["seed"], False)[0][0]
    xd = gpu(R.fixture_inputs(c["seed"], "a")[0])
    two = ["ts_conv3x3_s_fwd", "ts_fused_project_fwd"]
    cn, stem = ts.ConvBnAct(24, 24, skip=True).to(_dev()).eval(), ts.StemConv(24, 8).to(_dev()).eval()
    with torch.no_grad():
        with TF.WeightLayouts(), TF.BNFolds():
            first = m(xd)
            cn(xd), stem(xd)
            with _lib.Recorder() as rec:
                second = m(xd)
            assert [name for name, _ in rec.log] == two
            for blk in (cn, stem):
                with _lib.Recorder() as rec:
                    blk(xd)
                assert [name for name, _ in rec.log] == two[:1]
        with _lib.Recorder() as rec:
            bare = m(xd)
        assert sorted(name for name, _ in rec.log) == sorted(two + ["ts_conv3x3_s_weight_layout", "ts_mbconv_weight_layout"] + ["ts_bn_fold_many"] * 2)
        with _lib.Recorder() as rec:
            cn(xd)
        assert sorted(name for name, _ in rec.log) == sorted(two[:1] + ["ts_conv3x3_s_weight_layout", "ts_bn_fold_many"])
    assert same_bits(first, second) and same_bits(first, bare)


# ------------------------------------------------------------------------------------------------------------------ the whole backbone
def adopted_backbone(seed, training):
    theirs = R.StandInBackbone(layers.Conv2d)
    theirs.load_state_dict(R.fixture_state(seed, "d"), strict=True)
    theirs = theirs.to(_dev()).train(training)
    return ts.TemporalStereoBackbone.from_backbone(theirs), theirs


def test_whole_backbone_in_eval_mode():
    """Case d through TemporalStereoBackbone.from_backbone(stand-in) over two frames: the fixture's outputs; the bits of the walk by hand on
    a module built from the table; nothing is kept between calls."""
    seed = case("d", "eval")["seed"]
    net, theirs = adopted_backbone(seed, False)
    with torch.no_grad():
        got = device_run("d", "eval", net=net)
        by_hand = device_run("d", "eval", stages=True)
    assert set(got) == {"f%d_%s" % (f, k) for f in range(2) for k in R.OUTS}
    compare_forward("d", "eval", got, " (from_backbone)")
    for k in got:
        assert same_bits(got[k], by_hand[k]), k
    # the contexts forward opens live for one call: a weight written between calls -- in place, or through .data, which no version
    # counter sees -- is what the next call computes with
    with torch.no_grad():
        again = device_run("d", "eval", net=net)
        theirs.block1[0][0].conv_exp.weight.data.mul_(2.0)
        changed = device_run("d", "eval", net=net)
        theirs.block1[0][0].conv_exp.weight.data.mul_(0.5)
        theirs.bn1.running_var.data.mul_(4.0)
        folded = device_run("d", "eval", net=net)
        theirs.bn1.running_var.data.mul_(0.25)
        back = device_run("d", "eval", net=net)
    for k in got:
        assert same_bits(got[k], again[k]) and same_bits(got[k], back[k]), k
        assert not same_bits(got[k], changed[k]) and not same_bits(got[k], folded[k]), k


def test_whole_backbone_in_train_mode():
    seed = case("d", "train")["seed"]
    net, _ = adopted_backbone(seed, True)
    got = device_run("d", "train", net=net)
    compare_forward("d", "train", got, " (from_backbone)")
    compare_grads("d", got, " (from_backbone)")
