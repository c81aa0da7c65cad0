"""FeatureDecoder without a GPU: tests/decoder_ref.py (the plain-torch restatement, the fp64 yardstick of tests/test_decoder_gpu.py) and
temporalstereo_amd.FeatureDecoder on CPU tensors against the reference's own runs in tests/golden/decoder_*.npz (tools/gen_golden.py
--only-decoder); the constructor, state-dict and from_backbone contract; the argument checks of the new C-ABI entries (they come before
any launch).

Bars: the fixture's recorded deviation of the reference's fp32 run from its fp64 run.  decoder_ref in fp64 stands where the reference's
fp64 run stands (1e-10, asserted by the generator), so it lies within dev_* (+ 1e-9) of the stored fp32 values; decoder_ref in fp32 is
the reference's own op sequence and lies within dev_* of them too.  Gradients: relative L2 <= rel_grad_* (+ 1e-9) where the whole array is
stored; where 8192 seeded positions of a larger array are stored the ratio over those positions scatters around the whole array's by
~0.8 % (the root of a chi-square mean of 8192 terms), and 1.25 leaves that thirty-fold (as tests/test_conv_gru_cpu.py).
"""
import ctypes

import pytest
import torch
import torch.nn as nn

import decoder_ref as R
from compare import T, err, null_sweep, rel_l2
import temporalstereo_amd as ts
from temporalstereo_amd import _lib
from temporalstereo_amd import functional as TF
from temporalstereo_amd import layers

TAGS = ("a", "b")


def test_state_dict_is_the_references():
    g = R.load_fixture("a")
    m = ts.FeatureDecoder()
    assert list(m.state_dict().keys()) == g["keys"] == list(R.KEYS)
    assert [tuple(v.shape) for v in m.state_dict().values()] == g["key_shapes"] == [s for _, s in R.key_shapes()]
    state = R.fixture_state(g["seed"])
    res = m.load_state_dict(state, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in m.state_dict().items():
        assert torch.equal(v, state[k]), k
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in state.items() if k != "deconv8_4.1.weight"}, strict=True)
    for name in ("conv32", "deconv32_16", "deconv16_8", "deconv8_4"):
        for conv in ([m.conv32] if name == "conv32" else list(getattr(m, name))):
            assert isinstance(conv, layers.Conv2d) and conv.bias is None
            assert conv.kernel_size == (3, 3) and conv.padding == (1, 1) and conv.stride == (1, 1)
    assert isinstance(m.deconv16_8[0].norm, nn.BatchNorm2d) and isinstance(m.deconv16_8[0].activation, nn.SiLU)
    assert m.deconv16_8[1].norm is None and m.conv32.norm is None and m.conv32.activation is None
    assert ts.FeatureDecoder is ts.backbone.FeatureDecoder and ts.decoder_conv is TF.decoder_conv
    small = ts.FeatureDecoder(channels=(3, 4, 5, 6, 7), out_channels=(0, 32, 64, 96, 11), norm="GN", activation="ReLU")
    assert tuple(small.deconv8_4[0].weight.shape) == (32, 64 + 4, 3, 3) and isinstance(small.deconv8_4[0].norm, nn.GroupNorm)


@pytest.mark.parametrize("training", (True, False))
@pytest.mark.parametrize("tag", TAGS)
def test_cpu_forward_is_the_restatement_in_fp64(tag, training):
    g = R.load_fixture(tag)
    m = ts.FeatureDecoder()
    m.load_state_dict(R.fixture_state(g["seed"]), strict=True)
    m = m.double().train(training)
    maps = R.fixture_input(g["seed"], tag, torch.float64)
    want = R.decoder(maps["x4"], maps["x8"], maps["x16"], maps["x32"], R.fixture_state(g["seed"], torch.float64), training)
    with torch.no_grad():
        got = m(maps["x4"], maps["x8"], maps["x16"], maps["x32"])
        again = m._reference_forward(maps["x4"], maps["x8"], maps["x16"], maps["x32"])
    assert isinstance(got, list) and len(got) == 3
    for k, t, t2 in zip(R.OUTPUTS, got, again):
        assert t.shape == want[k].shape and err(t, want[k]) <= 1e-12, k
        assert err(t2, want[k]) <= 1e-12, k


@pytest.mark.parametrize("tag", TAGS)
def test_ref_reproduces_the_fixture(tag):
    g = R.load_fixture(tag)
    seed = g["seed"]
    for mode in R.MODES:
        r64 = R.run(seed, tag, torch.float64, mode == "train")
        for dt in (torch.float64, torch.float32):
            run = r64 if dt is torch.float64 else R.run(seed, tag, dt, mode == "train")
            for k in R.OUTPUTS:
                name = "%s_%s" % (mode, k)
                assert float(g["max_" + name]) == pytest.approx(float(r64[k].abs().max()), rel=1e-9)
                if name in g:
                    assert err(R.sample(run[k], seed), T(g[name])) <= float(g["dev_" + name]) + 1e-9, (tag, dt, name)
                if dt is torch.float32:       # the restatement in fp32 is the reference's op sequence: its deviation is the stored one's class
                    assert err(run[k], r64[k]) <= 2.0 * float(g["dev_" + name]) + 1e-9, (tag, name)
            for k in R.INPUTS + R.PARAM_KEYS:
                name = "grad_%s_%s" % (mode, k)
                if name not in g:
                    continue
                got, ref, want = R.sample(run["grad_" + k], seed), R.sample(r64["grad_" + k], seed), T(g[name])
                slack = 1.0 if R.sample_index(seed, run["grad_" + k].numel()) is None else 1.25
                assert rel_l2(got, want, ref) <= slack * float(g["rel_" + name]) + 1e-9, (tag, dt, name)


def test_fused_layer_of_the_restatement():
    """fused_layer with up=None is F.conv2d; with an identity resize it is the plain form on torch.cat."""
    up, skip = torch.randn(1, 4, 6, 6, dtype=torch.float64), torch.randn(1, 4, 6, 6, dtype=torch.float64)
    w = torch.randn(16, 8, 3, 3, dtype=torch.float64)
    assert torch.equal(R.fused_layer(None, skip, w[:, 4:]), torch.nn.functional.conv2d(skip, w[:, 4:], padding=1))
    assert err(R.fused_layer(up, skip, w), R.fused_layer(None, torch.cat([up, skip], 1), w)) <= 1e-14


class _Backbone(nn.Module):
    """What a reference backbone offers from_backbone: the four submodules among others."""

    def __init__(self, conv=layers.Conv2d):
        super().__init__()
        self.conv_stem = nn.Conv2d(3, 8, 3)
        self.norm, self.activation = 'BN', 'SiLU'
        c, o = (3, 4, 5, 6, 7), (0, 8, 9, 10, 11)

        def pair(cin, cout):
            first = conv(cin, cout, 3, 1, 1, bias=False)
            first.norm, first.activation = nn.BatchNorm2d(cout), nn.SiLU(inplace=True)
            second = conv(cout, cout, 3, 1, 1, bias=False)
            second.norm = second.activation = None
            return nn.Sequential(first, second)
        self.conv32 = conv(c[4], o[4], 3, 1, 1, bias=False)
        self.conv32.norm = self.conv32.activation = None
        self.deconv32_16, self.deconv16_8, self.deconv8_4 = pair(o[4] + c[3], o[3]), pair(o[3] + c[2], o[2]), pair(o[2] + c[1], o[1])


@pytest.mark.parametrize("conv", (layers.Conv2d, nn.Conv2d))
def test_from_backbone_shares_parameters(conv):
    bb = _Backbone(conv)
    dec = ts.FeatureDecoder.from_backbone(bb)
    own = dict(dec.named_parameters())
    theirs = {k: v for k, v in bb.named_parameters() if not k.startswith("conv_stem")}
    assert set(own) == set(theirs) and len(own) == 7 + 6
    for k in own:
        assert own[k] is theirs[k], k
    bufs, their_bufs = dict(dec.named_buffers()), dict(bb.named_buffers())
    for k in bufs:
        assert bufs[k] is their_bufs[k], k
    assert dec.channels == (0, 4, 5, 6, 7) and dec.out_channels == (0, 8, 9, 10, 11)
    x4, x8, x16, x32 = torch.randn(2, 4, 8, 12), torch.randn(2, 5, 4, 6), torch.randn(2, 6, 2, 3), torch.randn(2, 7, 1, 2)
    dec.eval()
    state = {k: v for k, v in bb.state_dict().items() if not k.startswith("conv_stem")}
    want = R.decoder(x4, x8, x16, x32, state, False)
    with torch.no_grad():
        got = dec(x4, x8, x16, x32)
    for k, t in zip(R.OUTPUTS, got):
        assert err(t, want[k]) <= 1e-5, k
    with pytest.raises(ValueError):
        ts.FeatureDecoder.from_backbone(nn.Sequential())


def test_forward_refuses_maps_that_do_not_belong_together():
    m = ts.FeatureDecoder(channels=(3, 4, 5, 6, 7), out_channels=(0, 8, 9, 10, 11))
    x4, x8, x16, x32 = torch.randn(2, 4, 8, 12), torch.randn(2, 5, 4, 6), torch.randn(2, 6, 2, 3), torch.randn(2, 7, 1, 2)
    m(x4, x8, x16, x32)
    with pytest.raises(ValueError, match="B,C,H,W"):
        m(x4[0], x8, x16, x32)
    with pytest.raises(ValueError, match="B,C,H,W"):
        m(x4, x8, x16, x32.unsqueeze(0))
    with pytest.raises(ValueError, match="batch"):
        m(x4, x8[:1], x16, x32)
    with pytest.raises(ValueError, match="batch"):
        m(x4, x8, x16, torch.cat([x32, x32]))
    with pytest.raises(ValueError, match="smaller"):
        m(x4, x8, x16, torch.randn(2, 7, 3, 2))
    with pytest.raises(ValueError, match="smaller"):
        m(x4[..., :5], x8, x16, x32)


def test_functional_refuses_cpu_tensors_and_bad_arguments():
    up, skip, w = torch.randn(1, 3, 2, 2), torch.randn(1, 2, 4, 4), torch.randn(6, 5, 3, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        TF.decoder_conv(up, skip, w)
    with pytest.raises(ValueError, match="activation"):
        TF.decoder_conv(up, skip, w, activation="ReLU")
    with pytest.raises(ValueError, match="BatchNorm"):
        TF.decoder_conv(up, skip, w, bn=nn.GroupNorm(2, 6))
    assert TF.decoder_conv_supported(512, 512) and TF.decoder_conv_supported(1, 1)
    assert not TF.decoder_conv_supported(513, 8) and not TF.decoder_conv_supported(8, 513) and not TF.decoder_conv_supported(0, 8)


def test_abi_version_and_argument_checks():
    L = _lib.lib()
    assert L.ts_version() >= 24
    buf = ctypes.create_string_buffer(64)
    one = (ctypes.addressof(buf) + 15) // 16 * 16        # never dereferenced by a call that is refused; 16-byte aligned
    far, farther = one + (1 << 40), one + (1 << 41)      # operands that overlap neither `one` nor one another
    big = 1 << 20

    # ts_decoder_weight_bytes(Cin, Cout) / ts_decoder_weight_layout(w, w_l, Cin, Cout, stream)
    assert L.ts_decoder_weight_bytes(17, 20) >= 17 * 20 * 9 * 4 and L.ts_decoder_weight_bytes(512, 512) >= 512 * 512 * 9 * 4
    assert L.ts_decoder_weight_bytes(480, 256) % 16 == 0
    assert L.ts_decoder_weight_bytes(513, 8) == 0 and L.ts_decoder_weight_bytes(8, 513) == 0 and L.ts_decoder_weight_bytes(0, 8) == 0
    fn = L.ts_decoder_weight_layout
    null_sweep(fn, (one, one, 17, 20, None), (0, 1), "weight_layout")
    assert fn(one, one, 0, 20, None) == -2 and fn(one, one, 17, -1, None) == -2
    assert fn(one, one, 513, 20, None) == -3 and fn(one, one, 17, 513, None) == -3
    assert fn(one, one + 4, 17, 20, None) == -4

    # ts_decoder_conv_fwd(up, skip, w_l, scale, shift, y, B, Cu, Cs, Cout, h, w, H, W, act, up_bs, up_cs, skip_bs, skip_cs, y_bs, y_cs, stream)
    fn = L.ts_decoder_conv_fwd
    n, N = 4 * 7, 9 * 13

    def ok(B=2, Cu=12, Cs=5, Cout=20, h=4, w=7, H=9, W=13, act=1, ub=None, uc=None, sb=None, sc=None, yb=None, yc=None, up=one, skip=one,
           scale=one, shift=one):
        uc = h * w if uc is None else uc
        sc = H * W if sc is None else sc
        yc = H * W if yc is None else yc
        ub = Cu * uc if ub is None else ub
        sb = Cs * sc if sb is None else sb
        yb = Cout * yc if yb is None else yb
        return (up, skip, one, scale, shift, one, B, Cu, Cs, Cout, h, w, H, W, act, ub, uc, sb, sc, yb, yc, None)
    null_sweep(fn, ok(), (0, 1, 2, 5), "decoder_conv_fwd")
    # scale / shift may be NULL, and so may up when Cu = 0: such a call gets past the pointer checks, to the
    # alignment check of w_l that follows them
    for kw in (dict(scale=None, shift=None), dict(Cu=0, up=None, h=0, w=0)):
        a = list(ok(**kw))
        a[2] = one + 4
        assert fn(*a) == -4, kw
    for bad in (dict(B=0), dict(Cu=-1), dict(Cs=-1), dict(Cs=0), dict(Cs=0, skip=None), dict(Cu=0, Cs=0), dict(Cout=0), dict(h=0), dict(w=0), dict(H=0), dict(W=-2),
                dict(act=2), dict(act=-1)):
        assert fn(*ok(**bad)) == -2, bad
    assert fn(*ok(uc=n - 1)) == -2 and b"overlap" in L.ts_last_error_string()
    assert fn(*ok(ub=12 * n - 1)) == -2 and fn(*ok(sc=N - 1)) == -2 and fn(*ok(sb=5 * N - 1)) == -2
    assert fn(*ok(yc=N - 1)) == -2 and fn(*ok(yb=20 * N - 1)) == -2
    assert fn(*ok(Cu=500, Cs=13)) == -3 and fn(*ok(Cu=0, Cs=513, up=None)) == -3 and fn(*ok(Cout=513)) == -3
    assert fn(*ok(Cu=500, Cs=12, Cout=512, up=None)) == -1              # the envelope's corner passes the envelope check
    assert fn(*ok(B=1, H=big, W=1)) == -3 and fn(*ok(B=1, H=1, W=big)) == -3 and fn(*ok(B=1, h=big, w=1)) == -3 and fn(*ok(B=1, h=1, w=big)) == -3
    # the order: sizes before the envelope before pointers
    assert fn(*ok(Cout=513, yc=N - 1, skip=None)) == -2 and fn(*ok(Cout=513, skip=None)) == -3
    # the overlap rules, after pointers and alignment: y (argument 5) apart from up and from skip
    def at(y, **kw):
        a = list(ok(**kw))
        a[5] = y
        return a
    assert fn(*at(one, up=far)) == -2 and b"y overlaps skip" in L.ts_last_error_string()              # an output over its own input
    assert fn(*at(one, skip=far)) == -2 and b"y overlaps up" in L.ts_last_error_string()
    assert fn(*at(farther + 4 * (2 * 5 * N - 1), up=far, skip=farther)) == -2                         # y begins on skip's last element
    assert fn(*at(far + 4 * (2 * 12 * n - 1), up=far, skip=farther)) == -2                            # ... on up's
    assert fn(*at(one, Cu=0, h=0, w=0)) == -2 and b"y overlaps skip" in L.ts_last_error_string()      # Cu = 0: `up` is not looked at
    a = at(one, up=far)
    a[2] = one + 4
    assert fn(*a) == -4                                                                               # after the alignment

    # ts_resize_bilinear_bwd(dy, dx, B, C, h, w, H, W, dy_bs, dy_cs, dx_bs, dx_cs, stream)
    fn = L.ts_resize_bilinear_bwd
    ok = lambda B=2, C=12, h=4, w=7, H=9, W=13, gb=17 * N, gc=N, xb=12 * n, xc=n: (one, one, B, C, h, w, H, W, gb, gc, xb, xc, None)
    null_sweep(fn, ok(), (0, 1), "resize_bilinear_bwd")
    for bad in (dict(B=0), dict(C=0), dict(h=0), dict(w=-1), dict(H=0), dict(W=0)):
        assert fn(*ok(**bad)) == -2, bad
    assert fn(*ok(gc=N - 1)) == -2 and b"overlap" in L.ts_last_error_string()
    assert fn(*ok(gb=12 * N - 1)) == -2 and fn(*ok(xc=n - 1)) == -2 and fn(*ok(xb=12 * n - 1)) == -2
    assert fn(*ok(B=1, H=big, gc=big * 13)) == -3 and fn(*ok(B=1, w=big, xc=big * 4)) == -3 and fn(*ok(B=1, C=big, gb=0, xb=0)) == -3


def test_sync_batchnorm_over_several_ranks_is_refused(monkeypatch):
    """functional.bn_exchanges, the rule FeatureDecoder routes by: a train-mode SyncBatchNorm whose group spans more than one rank (a
    patched torch.distributed) needs conv_bn_act's exchange; decoder_conv refuses it before anything else."""
    import torch.distributed as dist
    m = ts.FeatureDecoder(channels=(3, 4, 5, 6, 7), out_channels=(0, 8, 9, 10, 11), norm="SyncBN")
    sync, plain = m.deconv8_4[0].norm, nn.BatchNorm2d(8)
    assert isinstance(sync, nn.SyncBatchNorm)
    assert not TF.bn_exchanges(sync) and not TF.bn_exchanges(plain) and not TF.bn_exchanges(None)      # no process group initialised
    monkeypatch.setattr(dist, "is_initialized", lambda: True)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 1)
    assert not TF.bn_exchanges(sync)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
    assert TF.bn_exchanges(sync) and not TF.bn_exchanges(plain)
    up, skip = torch.randn(1, 9, 2, 2), torch.randn(1, 4, 4, 4)
    with pytest.raises(RuntimeError, match="SyncBatchNorm over 2 ranks"):
        TF.decoder_conv(up, skip, m.deconv8_4[0].weight, None, sync, "SiLU")
    sync.eval()
    assert not TF.bn_exchanges(sync)
    with pytest.raises(RuntimeError, match="no CPU fallback"):             # eval mode gets past the rule (and stops at the CPU tensors)
        TF.decoder_conv(up, skip, m.deconv8_4[0].weight, None, sync, "SiLU")
    with pytest.raises(ValueError, match="momentum"):
        TF.decoder_conv(up, skip, m.deconv8_4[0].weight, None, nn.BatchNorm2d(8, momentum=None), "SiLU")
    # (the module's routing by the same rule runs on the device: tests/test_decoder_gpu.py::test_sync_batchnorm_routing)
