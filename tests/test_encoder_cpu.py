"""The encoder's large planes and the Backbone module without a GPU: tests/encoder_ref.py (the plain-torch restatement, the fp64 yardstick
of tests/test_encoder_gpu.py) and temporalstereo_amd.StemConv / ConvBnAct / FusedInvertedResidual / TemporalStereoBackbone on CPU tensors
(their reference route) against the reference's own runs in tests/golden/encoder_*.npz (tools/gen_golden.py --only-encoder); the
constructor, state-dict, from_block and from_backbone contracts; routing decisions on CPU tensors; the argument checks of the new
C-ABI entries (they come before any launch).

Bars, those of tests/test_mbconv_cpu.py (argued there), with u = 2^-24:
  fp64 module against the fp64 restatement      1e-10 (relative to max |.|)
  an fp32 run against fp64                      max(2 dev, 16 u max |stage|);  gradients: relative L2 <= max(2 rel_grad, 1e-6)
  an fp32 run against the stored fp32 values    that plus dev (plus rel_grad): the triangle through fp64
  the fp64 restatement against stored values    dev (rel_grad; 1.25 times that where 8192 seeded positions of a larger array are stored)
"""
import ctypes

import pytest
import torch
import torch.nn as nn

import encoder_ref as R
from compare import T, err, fp32_bar, fp32_rel_bar, null_sweep, rel_l2
import temporalstereo_amd as ts
from temporalstereo_amd import _lib
from temporalstereo_amd import functional as TF
from temporalstereo_amd import layers

MP = R.MEMORY_PERCENT


def own_net(tag, seed, dtype=torch.float32, training=False):
    """The package's modules in the fixture's layout, with the fixture's state."""
    c = R.CASES[tag]
    if c["kind"] == "backbone":
        net = ts.TemporalStereoBackbone(arch=R.MINI, memory_percent=MP)
    else:
        net = nn.Sequential(nn.Sequential(*[ts.FusedInvertedResidual(cin, cout, stride=s, mid_chs=cmid) for cin, cmid, cout, s in c["members"]]))
    res = net.load_state_dict(R.fixture_state(seed, tag), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return net.to(dtype).train(training)


def module_run(tag, seed, dtype, training, net=None):
    """The package's module over the fixture's inputs on CPU tensors -> dict(f<frame>_<out | x4 | x8 | x16>, grad_*)"""
    c = R.CASES[tag]
    net = own_net(tag, seed, dtype, training) if net is None else net
    ins = [t.requires_grad_(True) for t in R.fixture_inputs(seed, tag, dtype)]
    res, outs = {}, []
    if c["kind"] == "backbone":
        info = {}
        for f in range(c["frames"]):
            l_fms, r_fms, info = net(ins[2 * f], ins[2 * f + 1], info)
            assert [m.shape[1] for m in info["memories"]] == [6, 8]
            for k, l, r in zip(R.OUTS, l_fms, r_fms):
                outs.append(torch.cat([l, r], 0))
                res["f%d_%s" % (f, k)] = outs[-1].detach()
    else:
        if c["kind"] == "stage":
            out, memories, idx = ts.block_forward(net, ins[0], MP, None, 0)
            assert memories == [] and idx == 0
        else:
            out = net[0][0](ins[0])
        outs.append(out)
        res["f0_out"] = out.detach()
    torch.autograd.backward(outs, R.fixture_cotangents(seed, tag, dtype))
    for name, x in zip(R.input_names(tag), ins):
        res["grad_" + name] = x.grad
    for k, p in net.named_parameters():
        res["grad_" + k] = p.grad
    return res


@pytest.mark.parametrize("tag", R.TAGS)
def test_state_dict_is_the_fixtures(tag):
    g = R.load_fixture(tag)
    net = own_net(tag, g["seed"])
    assert list(net.state_dict().keys()) == g["keys"] == [k for k, _ in R.key_shapes(tag)]
    assert [tuple(v.shape) for v in net.state_dict().values()] == g["key_shapes"]
    state = R.fixture_state(g["seed"], tag)
    for k, v in net.state_dict().items():
        assert torch.equal(v, state[k]), k
    with pytest.raises(RuntimeError):
        net.load_state_dict({k: v for k, v in state.items() if k != g["keys"][0]}, strict=True)


def test_modules_follow_the_timm_blocks_and_the_reference_layout():
    m = ts.FusedInvertedResidual(24, 48, stride=2)
    assert list(m.state_dict().keys())[:1] == ["conv_exp.weight"] and [k for k in m.state_dict() if "bn" not in k] == ["conv_exp.weight", "conv_pwl.weight"]
    assert m.conv_exp.out_channels == 96 and m.conv_exp.stride == (2, 2) and m.conv_exp.padding == (1, 1) and m.conv_exp.bias is None
    assert m.has_residual is False and m.drop_path_rate == 0.0 and isinstance(m.act1, nn.SiLU) and isinstance(m.se, nn.Identity)
    assert ts.FusedInvertedResidual(48, 48).has_residual is True and ts.FusedInvertedResidual(48, 48, noskip=True).has_residual is False
    assert ts.FusedInvertedResidual(64, 64).conv_exp.out_channels == 256
    cn = ts.ConvBnAct(24, 24, skip=True)
    assert [k for k in cn.state_dict() if "bn" not in k] == ["conv.weight"] and cn.has_residual is True
    assert ts.ConvBnAct(24, 32, skip=True).has_residual is False and ts.ConvBnAct(24, 24).has_residual is False
    assert list(ts.StemConv().state_dict().keys())[:2] == ["conv_stem.weight", "bn1.weight"] and ts.StemConv().conv_stem.stride == (2, 2)
    with pytest.raises(ValueError):
        ts.InvertedResidual(24, 24, 1)
    ir = ts.InvertedResidual(64, 128, 2)
    assert ir.conv_pw.out_channels == 256 and ir.conv_dw.stride == (2, 2) and ir.se.conv_reduce.out_channels == 16 and ir.has_residual is False
    assert ir(torch.zeros(1, 64, 6, 8)).shape == (1, 128, 3, 4)
    # the full layout: the reference's channels (backbone/TemporalStereo.py:74), its 27 memory blocks, its state-dict keys
    net = ts.TemporalStereoBackbone()
    keys = list(net.state_dict().keys())
    for k in ("conv_stem.weight", "bn1.running_var", "block0.0.0.conv.weight", "block0.0.1.bn1.weight", "block1.0.0.conv_exp.weight",
              "block1.0.3.conv_pwl.weight", "block2.0.3.bn2.bias", "block3.0.0.conv_dw.weight", "block3.1.8.se.conv_expand.bias",
              "block4.0.14.bn3.weight", "conv32.weight", "deconv32_16.0.norm.weight", "deconv8_4.1.weight"):
        assert k in keys, k
    assert not [k for k in keys if k.split(".")[0] not in ("conv_stem", "bn1", "block0", "block1", "block2", "block3", "block4", "conv32",
                                                            "deconv32_16", "deconv16_8", "deconv8_4")]
    assert [getattr(net, "block%d" % i)[-1][-1].state_dict()[w].shape[0] for i, w in enumerate(("conv.weight", "conv_pwl.weight", "conv_pwl.weight",
                                                                                                 "conv_pwl.weight", "conv_pwl.weight"))] == [24, 48, 64, 160, 272]
    members = [m for i in range(5) for seq in getattr(net, "block%d" % i) for m in seq]
    assert sum(isinstance(m, ts.MemoryInvertedResidual) for m in members) == 27 and sum(isinstance(m, ts.FusedInvertedResidual) for m in members) == 8
    assert sum(isinstance(m, ts.ConvBnAct) for m in members) == 2 and sum(type(m) is ts.InvertedResidual for m in members) == 3
    assert net.block1[0][0].conv_exp.weight.shape == (96, 24, 3, 3) and net.block2[0][0].conv_exp.weight.shape == (192, 48, 3, 3)
    assert net.memory_percent == 0.25 and net.conv32.weight.shape == (320, 272, 3, 3)
    assert ts.fused_mbconv_supported is TF.fused_mbconv_supported and ts.conv3x3_bn_act is TF.conv3x3_bn_act and ts.fused_mbconv_eval is TF.fused_mbconv_eval
    assert TF.fused_mbconv_supported(24, 96, 48, 2) and TF.fused_mbconv_supported(64, 256, 64, 1) and TF.fused_mbconv_supported(128, 512, 512, 2)
    assert not TF.fused_mbconv_supported(129, 8, 8, 2) and TF.fused_mbconv_supported(512, 8, 8, 1) and not TF.fused_mbconv_supported(513, 8, 8, 1)
    assert not TF.fused_mbconv_supported(8, 513, 8, 1) and not TF.fused_mbconv_supported(8, 8, 513, 1) and not TF.fused_mbconv_supported(8, 8, 8, 3)


@pytest.mark.parametrize("tag", R.TAGS)
def test_ref_reproduces_the_fixture(tag):
    g = R.load_fixture(tag)
    seed = g["seed"]
    for mode in R.MODES:
        r64 = R.run(seed, tag, torch.float64, mode == "train")
        for dt in (torch.float64, torch.float32):
            run = r64 if dt is torch.float64 else R.run(seed, tag, dt, mode == "train")
            for k in [k for k in r64 if not k.startswith("grad_")]:
                name = "%s_%s" % (mode, k)
                assert float(g["max_" + name]) == pytest.approx(float(r64[k].abs().max()), rel=1e-9)
                assert (name in g) == R.stored(name), name
                if name in g:
                    bar = float(g["dev_" + name]) + (0.0 if dt is torch.float64 else fp32_bar(g, name))
                    assert err(R.sample(run[k], seed), T(g[name])) <= bar + 1e-9, (tag, dt, name)
                if dt is torch.float32:
                    assert err(run[k], r64[k]) <= fp32_bar(g, name) + 1e-9, (tag, name)
            for k in [k for k in r64 if k.startswith("grad_")]:
                name = "grad_%s_%s" % (mode, k[5:])
                assert "rel_" + name in g
                if name not in g:
                    continue
                got, ref, want = R.sample(run[k], seed), R.sample(r64[k], seed), T(g[name])
                slack = 1.0 if R.sample_index(seed, run[k].numel()) is None else 1.25
                bar = float(g["rel_" + name]) + (0.0 if dt is torch.float64 else fp32_rel_bar(g, name))
                assert rel_l2(got, want, ref) <= slack * bar + 1e-9, (tag, dt, name)


@pytest.mark.parametrize("training", (True, False))
@pytest.mark.parametrize("tag", R.TAGS)
def test_cpu_module_is_the_restatement(tag, training):
    """The modules on CPU tensors (their reference route): fp64 equals the restatement to rounding; fp32 lies within the fixture's bars."""
    g = R.load_fixture(tag)
    seed, mode = g["seed"], "train" if training else "eval"
    r64 = R.run(seed, tag, torch.float64, training)
    got = module_run(tag, seed, torch.float64, training)
    assert set(got) == {k for k in r64 if k.startswith("grad_") or k.split("_", 1)[1] in ("out",) + R.OUTS}
    for k, v in got.items():
        assert v.shape == r64[k].shape and err(v, r64[k]) <= 1e-10 * max(1.0, float(r64[k].abs().max())), k
    got = module_run(tag, seed, torch.float32, training)
    for k, v in got.items():
        if k.startswith("grad_"):
            name = "grad_%s_%s" % (mode, k[5:])
            assert rel_l2(v, r64[k], r64[k]) <= fp32_rel_bar(g, name) + 1e-9, (tag, name)
        else:
            name = "%s_%s" % (mode, k)
            assert err(v, r64[k]) <= fp32_bar(g, name) + 1e-9, (tag, name)
            assert err(R.sample(v, seed), T(g[name])) <= float(g["dev_" + name]) + fp32_bar(g, name) + 1e-9, (tag, name)


def stand_in_backbone(seed, dtype=torch.float64):
    theirs = R.StandInBackbone(layers.Conv2d)
    theirs.load_state_dict(R.fixture_state(seed, "d"), strict=True)
    return theirs.to(dtype).eval()


def test_from_backbone_shares_parameters_and_runs_the_fixture():
    g = R.load_fixture("d")
    theirs = stand_in_backbone(g["seed"])
    net = ts.TemporalStereoBackbone.from_backbone(theirs)
    assert list(net.state_dict().keys()) == g["keys"] and net.training is False and net.memory_percent == MP
    mine, other = dict(net.named_parameters()), dict(theirs.named_parameters())
    assert set(mine) == set(other) and all(mine[k] is other[k] for k in mine)
    mine, other = dict(net.named_buffers()), dict(theirs.named_buffers())
    assert set(mine) == set(other) and all(mine[k] is other[k] for k in mine)
    assert isinstance(net.block0[0][0], ts.ConvBnAct) and net.block0[0][0].conv is theirs.block0[0][0].conv and net.block0[0][0].has_residual
    for name in ("block1", "block2"):
        for i in range(2):
            blk = getattr(net, name)[0][i]
            assert isinstance(blk, ts.FusedInvertedResidual) and blk._recognised and blk.conv_exp is getattr(theirs, name)[0][i].conv_exp
            assert blk.has_residual == (i == 1)
    for name in ("block3", "block4"):
        assert getattr(net, name)[0][0] is getattr(theirs, name)[0][0]                 # the non-residual MBConv block runs as it is
        blk = getattr(net, name)[0][1]
        assert isinstance(blk, ts.MemoryInvertedResidual) and blk._recognised and blk.memory_percent == MP
    stem, decoder = net._parts
    assert isinstance(stem, ts.StemConv) and stem.conv_stem is theirs.conv_stem and stem.bn1 is theirs.bn1 and stem._recognised
    assert isinstance(decoder, ts.FeatureDecoder) and decoder.conv32 is theirs.conv32 and decoder.deconv8_4[1] is theirs.deconv8_4[1]
    got = module_run("d", g["seed"], torch.float64, False, net=net)
    r64 = R.run(g["seed"], "d", torch.float64, False)
    for k, v in got.items():
        assert err(v, r64[k]) <= 1e-10 * max(1.0, float(r64[k].abs().max())), k
    # the stem and the decoder are views made per call: they follow the module's mode and leave a submodule's own mode alone
    net.train()
    theirs.deconv8_4[0].norm.eval()                                    # a frozen BatchNorm
    stem, decoder = net._parts
    assert stem.training and decoder.training and theirs.bn1.training and not theirs.deconv8_4[0].norm.training
    net.eval()
    stem, decoder = net._parts
    assert not stem.training and not decoder.training and not theirs.bn1.training
    with pytest.raises(ValueError):
        ts.TemporalStereoBackbone.from_backbone(nn.Sequential())


def test_forward_runs_the_submodules_registered_now():
    """A child replaced after construction is the one that runs: nn.SyncBatchNorm.convert_sync_batchnorm (what a trainer with
    sync_batchnorm does to the whole model), and plain assignments of `bn1` and `conv_stem`."""
    g = R.load_fixture("d")
    l, r = R.fixture_inputs(g["seed"], "d", torch.float64)[:2]
    for make in (lambda: own_net("d", g["seed"], torch.float64), lambda: ts.TemporalStereoBackbone.from_backbone(stand_in_backbone(g["seed"]))):
        net = make()
        with torch.no_grad():
            want = net(l, r, {})[0]
        old = net.bn1
        net = nn.SyncBatchNorm.convert_sync_batchnorm(net)
        stem, decoder = net._parts
        assert type(net.bn1) is nn.SyncBatchNorm and stem.bn1 is net.bn1 and stem.bn1 is not old and stem._recognised
        assert type(decoder.deconv8_4[0].norm) is nn.SyncBatchNorm and decoder.deconv8_4[0] is net.deconv8_4[0]
        assert all(type(m) is not nn.BatchNorm2d for m in net.modules())
        calls = []
        hook = net.bn1.register_forward_hook(lambda m, a, o: calls.append(type(m)))
        with torch.no_grad():
            got = net(l, r, {})[0]                                     # eval mode: a SyncBatchNorm is its running statistics
        hook.remove()
        assert calls == [nn.SyncBatchNorm] and all(torch.equal(a, b) for a, b in zip(got, want))

        class Marked(nn.BatchNorm2d):
            pass
        marked = Marked(net.bn1.num_features).double().eval()
        marked.load_state_dict(net.bn1.state_dict())
        net.bn1 = marked
        conv = nn.Conv2d(3, net.conv_stem.out_channels, 3, 2, 1, bias=False).double()
        with torch.no_grad():
            conv.weight.copy_(net.conv_stem.weight * 2.0)
        net.conv_stem = conv
        stem = net._parts[0]
        assert stem.bn1 is marked and stem.conv_stem is conv and not stem._recognised          # (a subclass of BatchNorm2d: the block's own submodules)
        hook = marked.register_forward_hook(lambda m, a, o: calls.append(type(m)))
        with torch.no_grad():
            changed = net(l, r, {})[0]
        hook.remove()
        assert calls[1:] == [Marked] and not torch.equal(changed[0], want[0])


def test_forward_is_the_references_contract():
    g = R.load_fixture("d")
    net = own_net("d", g["seed"], torch.float64)
    l, r = R.fixture_inputs(g["seed"], "d", torch.float64)[:2]
    with torch.no_grad():
        with pytest.raises(ValueError, match="expected input length 3"):
            net(l, r)
        l_fms, r_fms, info = net(l, r, {})
        assert [tuple(t.shape) for t in l_fms] == [(2, 8, 16, 24), (2, 12, 8, 12), (2, 16, 4, 6)] == [tuple(t.shape) for t in r_fms]
        # the memories are views of this frame's activations: the first mc channels of each residual MBConv block's input
        assert [tuple(m.shape) for m in info["memories"]] == [(4, 6, 4, 6), (4, 8, 2, 3)]
        assert all(m._base is not None for m in info["memories"])
        # a memory of the wrong width raises as the reference does
        bad = {"memories": [info["memories"][0][:, :5], info["memories"][1]]}
        with pytest.raises(AssertionError, match="memory shape"):
            net(l, r, bad)
        # memory_percent 0: no memories are kept, every block runs without one
        net.memory_percent = 0.0
        _, _, info0 = net(l, r, {"memories": []})
        assert info0["memories"] == []


def test_routing_on_cpu_tensors_and_recognition():
    g = R.load_fixture("a")
    x = R.fixture_inputs(g["seed"], "a")[0]
    blk = own_net("a", g["seed"])[0][0]
    assert blk._recognised and blk._route(x) == "reference" and blk._route(x.double()) == "reference"
    assert ts.ConvBnAct(24, 24, skip=True)._route(x) == "reference" and ts.StemConv(24, 8)._route(x) == "reference"
    calls = []
    real = ts.FusedInvertedResidual._reference_forward
    blk._reference_forward = lambda t: calls.append("reference") or real(blk, t)
    with torch.no_grad():
        want = blk(x)
    assert calls == ["reference"]

    def adopted(change):
        theirs = R.StandInEdge(24, 96, 24, 1)
        theirs.load_state_dict(blk.state_dict(), strict=True)
        change(theirs)
        return ts.FusedInvertedResidual.from_block(theirs.eval()), theirs
    same, theirs = adopted(lambda m: None)
    assert same._recognised and same.conv_exp is theirs.conv_exp and same.bn2 is theirs.bn2 and same.has_residual
    with torch.no_grad():
        assert torch.equal(same(x), want)

    class RealSE(nn.Module):
        def forward(self, t):
            return t * 0.5
    for name, change in (("se", lambda m: setattr(m, "se", RealSE())),
                         ("strided conv_pwl", lambda m: setattr(m, "conv_pwl", nn.Conv2d(96, 24, 1, 2, bias=False))),
                         ("activation", lambda m: setattr(m, "act1", nn.ReLU())),
                         ("norm", lambda m: setattr(m, "bn1", nn.GroupNorm(4, 96))),
                         ("5x5", lambda m: setattr(m, "conv_exp", nn.Conv2d(24, 96, 5, 1, 2, bias=False))),
                         ("bias", lambda m: setattr(m, "conv_exp", nn.Conv2d(24, 96, 3, 1, 1, bias=True)))):
        other, theirs = adopted(change)
        if name == "strided conv_pwl":
            other.has_residual = theirs.has_residual = False
        assert not other._recognised and other._route(x) == "reference", name
        with torch.no_grad():
            assert torch.equal(other(x), theirs(x)), name                  # the block's own submodules in the reference's order
    none_se, _ = adopted(lambda m: setattr(m, "se", None))                  # timm 0.4.12 leaves `se` None where there is none
    assert none_se._recognised
    with torch.no_grad():
        assert torch.equal(none_se(x), want)
    with pytest.raises(ValueError):
        ts.FusedInvertedResidual.from_block(nn.Identity())
    cn = ts.ConvBnAct.from_block(R.StandInConvBnAct(8, 8))
    assert cn._recognised and cn.has_residual
    odd = R.StandInConvBnAct(8, 8)
    odd.act1 = nn.ReLU()
    assert not ts.ConvBnAct.from_block(odd)._recognised
    assert not ts.StemConv.from_modules(nn.Conv2d(3, 8, 3, 2, 1, bias=True), nn.BatchNorm2d(8), nn.SiLU())._recognised


def test_drop_path_in_train_mode_takes_the_reference_route():
    blk = ts.FusedInvertedResidual(8, 8, drop_path_rate=0.5)
    x = torch.randn(4, 8, 5, 6)
    blk.train()
    torch.manual_seed(3)
    y = blk(x)
    blk.eval()
    with torch.no_grad():
        assert torch.equal(blk(x), blk._reference_forward(x))
    assert y.shape == x.shape


def test_abi_version_and_argument_checks():
    L = _lib.lib()
    assert L.ts_version() >= 23
    buf = ctypes.create_string_buffer(64)
    one = (ctypes.addressof(buf) + 15) // 16 * 16        # never dereferenced by a call that is refused; 16-byte aligned
    far = one + (1 << 40)                                # a second operand that does not overlap the first
    big = 1 << 20
    N, No = 9 * 13, 5 * 7

    # ts_conv3x3_s_weight_bytes(Cin, Cout, stride) / ts_conv3x3_s_weight_layout(w, w_l, Cin, Cout, stride, stream)
    assert L.ts_conv3x3_s_weight_bytes(24, 96, 1) >= 24 * 96 * 9 * 4 and L.ts_conv3x3_s_weight_bytes(24, 96, 2) >= 4 * 24 * 96 * 9 * 4
    assert L.ts_conv3x3_s_weight_bytes(3, 24, 2) % 16 == 0 and L.ts_conv3x3_s_weight_bytes(512, 512, 1) > 0 and L.ts_conv3x3_s_weight_bytes(128, 512, 2) > 0
    assert L.ts_conv3x3_s_weight_bytes(513, 8, 1) == 0 and L.ts_conv3x3_s_weight_bytes(129, 8, 2) == 0 and L.ts_conv3x3_s_weight_bytes(8, 513, 1) == 0
    assert L.ts_conv3x3_s_weight_bytes(8, 8, 3) == 0 and L.ts_conv3x3_s_weight_bytes(0, 8, 1) == 0
    fn = L.ts_conv3x3_s_weight_layout
    null_sweep(fn, (one, one, 24, 96, 2, None), (0, 1), "conv3x3_s_weight_layout")
    assert fn(one, one, 0, 96, 1, None) == -2 and fn(one, one, 24, -1, 1, None) == -2 and fn(one, one, 24, 96, 3, None) == -2
    assert fn(one, one, 513, 96, 1, None) == -3 and fn(one, one, 129, 96, 2, None) == -3 and fn(one, one, 24, 513, 1, None) == -3
    assert fn(one, one + 4, 24, 96, 1, None) == -4

    # ts_conv3x3_s_fwd(x, w_l, scale, shift, residual, y, B, Cin, Cout, H, W, stride, act, x_bs, x_cs, r_bs, r_cs, y_bs, y_cs, stream)
    fn = L.ts_conv3x3_s_fwd

    def ok(B=2, Cin=24, Cout=96, H=9, W=13, stride=1, act=1, xb=None, xc=None, rb=None, rcs=None, yb=None, yc=None, x=one, w_l=one, scale=one,
           shift=one, res=None, y=far):
        n = H * W
        no = ((H + 1) // 2) * ((W + 1) // 2) if stride == 2 else n
        xc = n if xc is None else xc
        rcs = no if rcs is None else rcs
        yc = no if yc is None else yc
        xb = Cin * xc if xb is None else xb
        rb = Cout * rcs if rb is None else rb
        yb = Cout * yc if yb is None else yb
        return (x, w_l, scale, shift, res, y, B, Cin, Cout, H, W, stride, act, xb, xc, rb, rcs, yb, yc, None)
    for stride in (1, 2):
        null_sweep(fn, ok(stride=stride), (0, 1, 5), "conv3x3_s_fwd")
        assert fn(*ok(stride=stride, w_l=one + 4, scale=None, shift=None)) == -4           # optional pointers: on to the alignment of w_l
    assert fn(*ok(res=one, w_l=one + 4)) == -4                                             # a residual at stride 1 is taken ...
    assert fn(*ok(res=one, stride=2)) == -2 and b"stride 1 only" in L.ts_last_error_string()            # ... at stride 2 refused
    for bad in (dict(B=0), dict(Cin=0), dict(Cout=-1), dict(H=0), dict(W=0), dict(stride=0), dict(stride=3), dict(act=2), dict(act=-1)):
        assert fn(*ok(**bad)) == -2, bad
    assert fn(*ok(xc=N - 1)) == -2 and b"overlap" in L.ts_last_error_string()
    assert fn(*ok(xb=24 * N - 1)) == -2 and fn(*ok(yc=N - 1)) == -2 and fn(*ok(yb=96 * N - 1)) == -2
    assert fn(*ok(res=one, rcs=N - 1)) == -2 and fn(*ok(res=one, rb=96 * N - 1)) == -2
    assert fn(*ok(stride=2, yc=No - 1)) == -2 and fn(*ok(stride=2, yc=No, yb=96 * No, w_l=one + 4)) == -4     # the output plane is (5, 7)
    assert fn(*ok(Cin=513)) == -3 and fn(*ok(Cin=129, stride=2)) == -3 and fn(*ok(Cout=513)) == -3
    assert fn(*ok(Cin=512, Cout=512, x=None)) == -1 and fn(*ok(Cin=128, stride=2, x=None)) == -1      # the envelope's corners pass the envelope check
    assert fn(*ok(B=1, H=big, W=1)) == -3 and fn(*ok(B=1, H=1, W=big)) == -3 and fn(*ok(B=big, H=1, W=1)) == -3
    assert fn(*ok(Cout=513, yc=N - 1, x=None)) == -2 and fn(*ok(Cout=513, x=None)) == -3              # sizes before the envelope before pointers
    assert fn(*ok(y=one)) == -2 and b"y overlaps x" in L.ts_last_error_string()                       # an output over its own input
    assert fn(*ok(y=one + 4 * (2 * 24 * N - 1))) == -2                                                # y begins on x's last element
    assert fn(*ok(res=far + 4)) == -2 and b"residual" in L.ts_last_error_string()                     # a residual shifted against y
    assert fn(*ok(res=far, rcs=N + 1)) == -2                                                          # the same pointer, other strides

    # ts_fused_project_fwd(x, w_l, scale, shift, residual, y, B, Cmid, Cout, H, W, x_bs, x_cs, r_bs, r_cs, y_bs, y_cs, stream)
    fn = L.ts_fused_project_fwd

    def ok(B=2, Cmid=96, Cout=24, H=9, W=13, xb=None, xc=None, rb=None, rcs=None, yb=None, yc=None, x=one, w_l=one, scale=one, shift=one,
           res=one, y=far):
        n = H * W
        xc = n if xc is None else xc
        rcs = n if rcs is None else rcs
        yc = n if yc is None else yc
        xb = Cmid * xc if xb is None else xb
        rb = Cout * rcs if rb is None else rb
        yb = Cout * yc if yb is None else yb
        return (x, w_l, scale, shift, res, y, B, Cmid, Cout, H, W, xb, xc, rb, rcs, yb, yc, None)
    null_sweep(fn, ok(), (0, 1, 5), "fused_project_fwd")
    assert fn(*ok(w_l=one + 4, scale=None, shift=None, res=None)) == -4
    for bad in (dict(B=0), dict(Cmid=0), dict(Cout=0), dict(H=-1), dict(W=0)):
        assert fn(*ok(**bad)) == -2, bad
    assert fn(*ok(xc=N - 1)) == -2 and b"overlap" in L.ts_last_error_string()
    assert fn(*ok(xb=96 * N - 1)) == -2 and fn(*ok(rcs=N - 1)) == -2 and fn(*ok(rb=24 * N - 1)) == -2
    assert fn(*ok(res=None, rcs=0, rb=0, w_l=one + 4)) == -4                                          # no residual: its strides are not looked at
    assert fn(*ok(yc=N - 1)) == -2 and fn(*ok(yb=24 * N - 1)) == -2
    assert fn(*ok(Cout=513)) == -3 and fn(*ok(Cmid=2049)) == -3 and fn(*ok(Cout=512, Cmid=2048, x=None)) == -1
    assert fn(*ok(B=1, H=big, W=1)) == -3 and fn(*ok(B=1, H=1, W=big)) == -3 and fn(*ok(B=1, H=60000, W=60000)) == -3
    assert fn(*ok(Cout=513, yc=N - 1, x=None)) == -2 and fn(*ok(Cout=513, x=None)) == -3
    assert fn(*ok(y=one)) == -2 and b"y overlaps x" in L.ts_last_error_string()
    assert fn(*ok(x=far + (1 << 30), res=far + 4)) == -2 and b"residual" in L.ts_last_error_string()
