"""MemoryInvertedResidual without a GPU: tests/mbconv_ref.py (the plain-torch restatement, the fp64 yardstick of tests/test_mbconv_gpu.py)
and temporalstereo_amd.MemoryInvertedResidual / block_forward on CPU tensors against the reference's own runs in tests/golden/mbconv_*.npz
(tools/gen_golden.py --only-mbconv); the constructor, state-dict and from_block contract; the argument checks of the new C-ABI entries
(they come before any launch).

Bars, as tests/test_decoder_cpu.py: the fixture's recorded deviation of the reference's fp32 run from its fp64 run.  mbconv_ref in fp64
stands where the reference's fp64 run stands (1e-10, asserted by the generator), so it lies within dev_* (+ 1e-9) of the stored fp32
values; mbconv_ref in fp32 is the reference's own op sequence and lies within 2 dev_* of its fp64 run.  Gradients: relative L2 <=
rel_grad_* (+ 1e-9) where the whole array is stored, 1.25 times that where 8192 seeded positions of a larger array are (the scatter of a
ratio over a sample, argued in tests/test_decoder_cpu.py).
An fp32 run of the restatement is not the fixture's fp32 run to the bit: the framework's CPU convolutions sum in an order that
depends on the processor and the thread count, and dev_* -- a maximum over as few as 544 values -- is one draw of a quantity that
varies with that order.  So the decoder's literal bars (an fp32 run within dev_* of the stored values, within 2 dev_* of fp64) hold
for one summation order only.  What holds for every order, with u = 2^-24:
  an fp32 run against fp64      max(2 dev, 16 u max |stage|): the decoder's 2 dev with the floor of tests/test_mbconv_gpu.py's stage bar
                                (gradients: relative L2 <= max(2 rel_grad, 1e-6), that file's floor);
  an fp32 run against stored    that plus dev (plus rel_grad): the triangle through fp64.
The fp64 comparisons keep the decoder's bars as they are.
"""
import ctypes

import pytest
import torch
import torch.nn as nn

import mbconv_ref as R
from compare import T, err, fp32_bar, fp32_rel_bar, null_sweep, rel_l2
import temporalstereo_amd as ts
from temporalstereo_amd import _lib
from temporalstereo_amd import functional as TF

MP = R.MEMORY_PERCENT


def own_stage(tag, seed, dtype=torch.float32, training=False):
    """The package's modules in the fixture's stage layout, with the fixture's state."""
    c = R.CASES[tag]
    net = nn.Sequential(nn.Sequential(*[ts.MemoryInvertedResidual(c["C"], mid_chs=c["Cmid"], se_chs=c["Cr"], memory_percent=MP)
                                        for _ in range(c["blocks"])]))
    res = net.load_state_dict(R.fixture_state(seed, tag), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return net.to(dtype).train(training)


def test_state_dict_is_the_references():
    g = R.load_fixture("a")
    c = R.CASES["a"]
    m = ts.MemoryInvertedResidual(c["C"], mid_chs=c["Cmid"], se_chs=c["Cr"])
    want = R.block_key_shapes(c["C"], c["Cmid"], c["Cr"])
    assert list(m.state_dict().keys()) == [k for k, _ in want] == [k[4:] for k in g["keys"]]
    assert [tuple(v.shape) for v in m.state_dict().values()] == [s for _, s in want] == g["key_shapes"]
    assert [k for k in m.state_dict() if not k.startswith("bn")] == ["conv_pw.weight", "conv_dw.weight", "se.conv_reduce.weight", "se.conv_reduce.bias",
                                                                     "se.conv_expand.weight", "se.conv_expand.bias", "conv_pwl.weight"]
    state = R.block_state(R.fixture_state(g["seed"], "a"))
    res = m.load_state_dict(state, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in m.state_dict().items():
        assert torch.equal(v, state[k]), k
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in state.items() if k != "se.conv_expand.bias"}, strict=True)
    assert m.has_residual is True and m.drop_path_rate == 0.0 and m.memory_percent == 0.25
    assert isinstance(m.act1, nn.SiLU) and isinstance(m.act2, nn.SiLU) and isinstance(m.se.act1, nn.SiLU) and isinstance(m.se.gate, nn.Sigmoid)
    assert m.conv_dw.groups == c["Cmid"] and m.conv_dw.padding == (1, 1) and m.conv_pw.bias is None and m.conv_pwl.bias is None
    assert ts.MemoryInvertedResidual is ts.backbone.MemoryInvertedResidual and ts.block_forward is ts.backbone.block_forward
    assert ts.depthwise_conv3x3 is TF.depthwise_conv3x3
    # the constructor's defaults are the EfficientNetV2 stages' widths
    for C, ratio, mid, se in ((128, 4.0, 512, 32), (160, 6.0, 960, 40), (272, 6.0, 1632, 68)):
        d = ts.MemoryInvertedResidual(C, exp_ratio=ratio)
        assert d.conv_pw.out_channels == mid and d.se.conv_reduce.out_channels == se


@pytest.mark.parametrize("tag", R.TAGS)
def test_ref_reproduces_the_fixture(tag):
    g = R.load_fixture(tag)
    seed = g["seed"]
    assert g["keys"] == [k for k, _ in R.key_shapes(tag)] and g["key_shapes"] == [s for _, s in R.key_shapes(tag)]
    for mode in R.MODES:
        r64 = R.run(seed, tag, torch.float64, mode == "train")
        for dt in (torch.float64, torch.float32):
            run = r64 if dt is torch.float64 else R.run(seed, tag, dt, mode == "train")
            for k in [k for k in r64 if not k.startswith("grad_")]:
                name = "%s_%s" % (mode, k)
                assert float(g["max_" + name]) == pytest.approx(float(r64[k].abs().max()), rel=1e-9)
                assert (name in g) == R.stored(name)
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


def module_run(tag, seed, dtype, training):
    """ts.block_forward over the fixture's frames on CPU tensors -> dict(f<frame>_out, grad_*)"""
    c = R.CASES[tag]
    net = own_stage(tag, seed, dtype, training)
    ins = [t.requires_grad_(True) for t in R.fixture_inputs(seed, tag, dtype)]
    memory = R.fixture_memory(seed, tag, dtype)
    if memory is not None:
        memory.requires_grad_(True)
    memories = [memory] if memory is not None else None
    res, outs = {}, []
    for f, x in enumerate(ins):
        out, memories, idx = ts.block_forward(net, x, MP, memories, 0)
        assert idx == c["blocks"] and len(memories) == c["blocks"]
        outs.append(out)
        res["f%d_out" % f] = out.detach()
    torch.autograd.backward(outs, R.fixture_cotangents(seed, tag, dtype))
    for f, x in enumerate(ins):
        res["grad_in_f%d" % f] = x.grad
    if memory is not None:
        res["grad_memory"] = memory.grad
    for k, p in net.named_parameters():
        res["grad_" + k] = p.grad
    return res


@pytest.mark.parametrize("training", (True, False))
@pytest.mark.parametrize("tag", R.TAGS)
def test_cpu_module_is_the_restatement(tag, training):
    """The module on CPU tensors (its reference path): fp64 equals the restatement to rounding; fp32 lies within the fixture's bars."""
    g = R.load_fixture(tag)
    seed, mode = g["seed"], "train" if training else "eval"
    r64 = R.run(seed, tag, torch.float64, training)
    got = module_run(tag, seed, torch.float64, training)
    assert set(got) == {k for k in r64 if k.startswith("grad_") or k.endswith("_out")}
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


def test_from_block_shares_parameters_and_runs_the_fixture():
    g = R.load_fixture("a")
    c = R.CASES["a"]
    theirs = R.StandInBlock(c["C"], c["Cmid"], c["Cr"])
    theirs.load_state_dict(R.block_state(R.fixture_state(g["seed"], "a")), strict=True)
    theirs.eval()
    m = ts.MemoryInvertedResidual.from_block(theirs, MP)
    assert m._recognised and not m.training and m.memory_percent == MP and m.has_residual
    own, want = dict(m.named_parameters()), dict(theirs.named_parameters())
    assert set(own) == set(want) and len(own) == 13
    for k in own:
        assert own[k] is want[k], k
    bufs, their_bufs = dict(m.named_buffers()), dict(theirs.named_buffers())
    assert set(bufs) == set(their_bufs) and len(bufs) == 9
    for k in bufs:
        assert bufs[k] is their_bufs[k], k
    x, memory = R.fixture_inputs(g["seed"], "a")[0], R.fixture_memory(g["seed"], "a")
    with torch.no_grad():
        out, new_memory = m(x, memory)
    assert new_memory.data_ptr() == x.data_ptr() and torch.equal(new_memory, x[:, :6])
    assert err(R.sample(out, g["seed"]), T(g["eval_f0_out"])) <= float(g["dev_eval_f0_out"]) + fp32_bar(g, "eval_f0_out") + 1e-9
    with pytest.raises(ValueError, match="conv_pw"):
        ts.MemoryInvertedResidual.from_block(nn.Sequential(), MP)
    theirs.has_residual = False
    with pytest.raises(ValueError, match="residual"):
        ts.MemoryInvertedResidual.from_block(theirs, MP)


class _Marker(nn.Module):
    """An activation the kernels do not compute: relu, and a record that the block's own submodule ran."""

    def __init__(self, log, name):
        super().__init__()
        self.log, self.name = log, name

    def forward(self, x):
        self.log.append(self.name)
        return torch.relu(x)


def test_from_block_routes_an_unrecognised_block_to_its_own_submodules():
    c = R.CASES["a"]
    make = lambda: R.StandInBlock(c["C"], c["Cmid"], c["Cr"]).eval()
    assert ts.MemoryInvertedResidual.from_block(make(), MP)._recognised
    log = []
    odd = make()
    odd.act2 = _Marker(log, "act2")
    m = ts.MemoryInvertedResidual.from_block(odd, MP)
    assert not m._recognised and m.act2 is odd.act2
    x, memory = torch.randn(2, c["C"], 5, 7), torch.randn(2, 6, 5, 7)
    assert m._route(x, memory) == "reference"
    with torch.no_grad():
        out, _ = m(x, memory)
        z = torch.cat([memory, x[:, 6:]], 1)
        z = odd.act1(odd.bn1(odd.conv_pw(z)))
        z = torch.relu(odd.bn2(odd.conv_dw(z)))
        want = x + odd.bn3(odd.conv_pwl(odd.se(z)))
    assert log == ["act2"] and err(out, want) <= 1e-6
    # every departure from the kernels' block is noticed
    for change in (lambda b: setattr(b, "act1", nn.ReLU()), lambda b: setattr(b, "bn2", nn.GroupNorm(4, c["Cmid"])),
                   lambda b: setattr(b, "bn3", nn.BatchNorm2d(c["C"], affine=False)), lambda b: setattr(b.se, "act1", nn.ReLU()),
                   lambda b: setattr(b.se, "gate", nn.Hardsigmoid()), lambda b: setattr(b, "conv_dw", nn.Conv2d(c["Cmid"], c["Cmid"], 3, 1, 1)),
                   lambda b: setattr(b, "conv_dw", nn.Conv2d(c["Cmid"], c["Cmid"], 5, 1, 2, groups=c["Cmid"], bias=False)),
                   lambda b: setattr(b, "conv_pw", nn.Conv2d(c["C"], c["Cmid"], 1, bias=True)),
                   lambda b: setattr(b.se, "conv_reduce", nn.Conv2d(c["Cmid"], c["Cr"], 1, bias=False))):
        b = make()
        change(b)
        assert not ts.MemoryInvertedResidual.from_block(b, MP)._recognised
    b = make()
    del b.se.gate
    b.se.gate = torch.sigmoid            # a function named sigmoid is the gate too
    assert ts.MemoryInvertedResidual.from_block(b, MP)._recognised


def test_block_forward_memory_indexing_over_two_frames():
    """A stage with a member that is no memory block between two that are: the memories are indexed by the memory blocks alone, the
    index carries over stages, and the second frame reads what the first frame returned."""
    C = 8
    blk = lambda: ts.MemoryInvertedResidual(C, mid_chs=16, se_chs=2, memory_percent=MP).eval()
    stage1 = nn.Sequential(nn.Sequential(blk(), nn.Conv2d(C, C, 1), blk()))
    stage2 = nn.Sequential(nn.Sequential(blk()), nn.Sequential(nn.Identity(), blk()))
    seen = []
    for m in list(stage1.modules()) + list(stage2.modules()):
        if isinstance(m, ts.MemoryInvertedResidual):
            real = m._forward
            m._forward = lambda x, mem, mp, real=real, m=m: seen.append((m, None if mem is None else mem)) or real(x, mem, mp)
    x0, x1 = torch.randn(1, C, 4, 5), torch.randn(1, C, 4, 5)
    with torch.no_grad():
        y, mem_a, idx = ts.block_forward(stage1, x0, MP, None, 0)
        assert idx == 2 and len(mem_a) == 2 and all(m.shape == (1, 2, 4, 5) for m in mem_a)
        assert torch.equal(mem_a[0], x0[:, :2])
        y, mem_b, idx = ts.block_forward(stage2, y, MP, [], idx)
        assert idx == 4 and len(mem_b) == 2
        assert all(mem is None for _, mem in seen) and len(seen) == 4
        first = mem_a + mem_b
        del seen[:]
        y, out_a, idx = ts.block_forward(stage1, x1, MP, first, 0)
        y, out_b, idx = ts.block_forward(stage2, y, MP, first, idx)
        assert idx == 4 and len(seen) == len(first) == 4 and all(a is b for (_, a), b in zip(seen, first))
        assert torch.equal(out_a[0], x1[:, :2])
        # memory_percent 0: the blocks are called plainly, nothing is collected
        y, none, idx = ts.block_forward(stage1, x0, 0.0, None, 0)
        assert none == [] and idx == 0 and y.shape == x0.shape


def test_wrong_width_memory_raises_the_references_text():
    m = ts.MemoryInvertedResidual(24, mid_chs=96, se_chs=6).eval()
    x = torch.randn(2, 24, 5, 7)
    with pytest.raises(AssertionError) as e:
        m(x, torch.randn(2, 5, 5, 7))
    assert str(e.value) == "input shape: {}; memory shape: {}!".format(x.shape, torch.Size((2, 5, 5, 7)))
    with pytest.raises(AssertionError, match="memory shape"):
        R.block(x, torch.randn(2, 7, 5, 7), R.block_state(R.fixture_state(1, "a")), False)
    m(x, torch.randn(2, 6, 5, 7))


def test_drop_path_in_train_mode_takes_the_reference_path(monkeypatch):
    m = ts.MemoryInvertedResidual(8, mid_chs=16, se_chs=2, drop_path_rate=0.5)
    calls = []
    monkeypatch.setattr(ts.backbone, "_drop_path", lambda x, rate, training: calls.append((rate, training)) or x)
    m.train()(torch.randn(2, 8, 3, 3))
    m.eval()(torch.randn(2, 8, 3, 3))
    assert calls == [(0.5, True), (0.5, False)]
    assert TF.mbconv_supported(512, 2048, 512) and TF.mbconv_supported(1, 1, 1)
    assert not TF.mbconv_supported(513, 8, 8) and not TF.mbconv_supported(8, 2049, 8) and not TF.mbconv_supported(8, 8, 513) and not TF.mbconv_supported(0, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        TF.depthwise_conv3x3(torch.randn(1, 4, 3, 3), torch.randn(4, 1, 3, 3))


def test_memory_and_operands_that_do_not_fit_the_input_raise():
    """A memory of another batch or plane (a stale one after the batch size changed) raises on every path, as the reference's
    torch.cat does; functional.mbconv_eval checks every operand's shape before any launch (CPU tensors get that far)."""
    m = ts.MemoryInvertedResidual(24, mid_chs=96, se_chs=6).eval()
    x = torch.randn(2, 24, 5, 7)
    for bad in (torch.randn(1, 6, 5, 7), torch.randn(3, 6, 5, 7), torch.randn(2, 6, 5, 8), torch.randn(2, 6, 4, 7), torch.randn(2, 6, 35)):
        with pytest.raises(RuntimeError, match="does not match"):
            m(x, bad)
        with pytest.raises(RuntimeError, match="does not match"):
            m.train()(x, bad)
        m.eval()
    fold = lambda n: (torch.ones(n), torch.zeros(n))

    def args(**kw):
        a = dict(inp=x, memory=torch.randn(2, 6, 5, 7), w_pw=m.conv_pw.weight, fold1=fold(96), w_dw=m.conv_dw.weight, fold2=fold(96),
                 w_reduce=m.se.conv_reduce.weight, b_reduce=m.se.conv_reduce.bias, w_expand=m.se.conv_expand.weight,
                 b_expand=m.se.conv_expand.bias, w_pwl=m.conv_pwl.weight, fold3=fold(24))
        a.update(kw)
        return a
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # every shape fits: on to the device check
        TF.mbconv_eval(**args())
    for kw, what in ((dict(memory=torch.randn(1, 6, 5, 7)), "memory"), (dict(memory=torch.randn(2, 6, 5, 6)), "memory"),
                     (dict(memory=torch.randn(2, 25, 5, 7)), "memory"), (dict(inp=x[0]), "input"), (dict(w_pw=torch.randn(96, 23, 1, 1)), "conv_pw"),
                     (dict(w_dw=torch.randn(96, 1, 5, 5)), "conv_dw"), (dict(w_reduce=torch.randn(6, 95, 1, 1)), "conv_reduce weight"),
                     (dict(b_reduce=torch.randn(5)), "conv_reduce bias"), (dict(w_expand=torch.randn(96, 5, 1, 1)), "conv_expand weight"),
                     (dict(b_expand=None), "conv_expand bias"), (dict(w_pwl=torch.randn(24, 97, 1, 1)), "conv_pwl"),
                     (dict(fold1=fold(95)), "bn1"), (dict(fold2=(torch.ones(96), None)), "bn2"), (dict(fold3=fold(23)), "bn3"),
                     (dict(out=torch.empty(2, 24, 5, 8)), "out"), (dict(out=torch.empty(2, 24, 7, 5).transpose(2, 3)), "out"),
                     (dict(out=torch.empty(4000).as_strided((2, 24, 5, 7), (35, 35, 7, 1))), "out")):          # overlapping batch elements
        with pytest.raises(ValueError, match=what):
            TF.mbconv_eval(**args(**kw))
    wide = ts.MemoryInvertedResidual(516, mid_chs=8, se_chs=2)
    with pytest.raises(RuntimeError, match="outside the kernel path"):
        TF.mbconv_eval(torch.randn(1, 516, 2, 2), None, wide.conv_pw.weight, fold(8), wide.conv_dw.weight, fold(8), wide.se.conv_reduce.weight,
                       wide.se.conv_reduce.bias, wide.se.conv_expand.weight, wide.se.conv_expand.bias, wide.conv_pwl.weight, fold(516))


def test_abi_version_and_argument_checks():
    L = _lib.lib()
    assert L.ts_version() >= 24
    buf = ctypes.create_string_buffer(64)
    one = (ctypes.addressof(buf) + 15) // 16 * 16        # never dereferenced by a call that is refused; 16-byte aligned
    far, farther = one + (1 << 40), one + (1 << 41)      # operands that overlap neither `one` nor one another
    big = 1 << 20
    N = 9 * 13

    # ts_mbconv_weight_bytes(Cin, Cout) / ts_mbconv_weight_layout(w, w_l, Cin, Cout, stream)
    assert L.ts_mbconv_weight_bytes(17, 20) >= 17 * 20 * 4 and L.ts_mbconv_weight_bytes(2048, 512) >= 2048 * 512 * 4
    assert L.ts_mbconv_weight_bytes(160, 960) % 16 == 0
    assert L.ts_mbconv_weight_bytes(2049, 8) == 0 and L.ts_mbconv_weight_bytes(8, 2049) == 0 and L.ts_mbconv_weight_bytes(0, 8) == 0
    fn = L.ts_mbconv_weight_layout
    null_sweep(fn, (one, one, 17, 20, None), (0, 1), "weight_layout")
    assert fn(one, one, 0, 20, None) == -2 and fn(one, one, 17, -1, None) == -2
    assert fn(one, one, 2049, 20, None) == -3 and fn(one, one, 17, 2049, None) == -3
    assert fn(one, one + 4, 17, 20, None) == -4

    # ts_mbconv_expand_fwd(memory, input, w_l, scale, shift, y, B, C, mc, Cmid, H, W, mem_bs, mem_cs, in_bs, in_cs, y_bs, y_cs, stream)
    fn = L.ts_mbconv_expand_fwd

    def ok(B=2, C=24, mc=6, Cmid=96, H=9, W=13, mb=None, mcs=None, ib=None, ics=None, yb=None, yc=None, memory=one, inp=one, w_l=one,
           scale=one, shift=one, y=one):
        n = H * W
        mcs = n if mcs is None else mcs
        ics = n if ics is None else ics
        yc = n if yc is None else yc
        mb = mc * mcs if mb is None else mb
        ib = C * ics if ib is None else ib
        yb = Cmid * yc if yb is None else yb
        return (memory, inp, w_l, scale, shift, y, B, C, mc, Cmid, H, W, mb, mcs, ib, ics, yb, yc, None)
    null_sweep(fn, ok(), (1, 2, 5), "expand_fwd")
    for kw in (dict(scale=None, shift=None), dict(memory=None), dict(memory=None, mb=0, mcs=0)):      # optional pointers: on to the alignment of w_l
        assert fn(*ok(w_l=one + 4, **kw)) == -4, kw
    for bad in (dict(B=0), dict(C=0), dict(Cmid=-1), dict(H=0), dict(W=0), dict(mc=-1), dict(mc=25)):
        assert fn(*ok(**bad)) == -2, bad
    assert fn(*ok(mcs=N - 1)) == -2 and b"overlap" in L.ts_last_error_string()
    assert fn(*ok(mb=6 * N - 1)) == -2 and fn(*ok(ics=N - 1)) == -2 and fn(*ok(ib=24 * N - 1)) == -2
    assert fn(*ok(yc=N - 1)) == -2 and fn(*ok(yb=96 * N - 1)) == -2
    assert fn(*ok(C=513)) == -3 and fn(*ok(Cmid=2049)) == -3
    assert fn(*ok(C=512, mc=128, Cmid=2048, inp=None)) == -1                   # the envelope's corner passes the envelope check
    assert fn(*ok(B=1, H=big, W=1)) == -3 and fn(*ok(B=1, H=1, W=big)) == -3 and fn(*ok(B=1, H=60000, W=60000)) == -3
    assert fn(*ok(Cmid=2049, yc=N - 1, inp=None)) == -2 and fn(*ok(Cmid=2049, inp=None)) == -3      # sizes before the envelope before pointers
    # the overlap rules, after pointers and alignment: y apart from memory and from input
    assert fn(*ok(memory=far, y=one)) == -2 and b"y overlaps input" in L.ts_last_error_string()        # an output over its own input
    assert fn(*ok(inp=far, y=one)) == -2 and b"y overlaps memory" in L.ts_last_error_string()
    assert fn(*ok(memory=far, inp=farther, y=farther + 4 * (2 * 24 * N - 1))) == -2                    # y begins on the input's last element
    assert fn(*ok(memory=far, inp=farther, y=far + 4 * (2 * 6 * N - 1))) == -2                         # ... on the memory's
    assert fn(*ok(memory=None, inp=far, y=far, w_l=one + 4)) == -4 and fn(*ok(memory=None, inp=far, y=far)) == -2      # after the alignment

    # ts_mbconv_project_fwd(x, gate, w_l, scale, shift, residual, y, B, Cmid, C, H, W, x_bs, x_cs, r_bs, r_cs, y_bs, y_cs, stream)
    fn = L.ts_mbconv_project_fwd

    def ok(B=2, Cmid=96, C=24, H=9, W=13, xb=None, xc=None, rb=None, rcs=None, yb=None, yc=None, x=one, gate=one, w_l=one, scale=one,
           shift=one, res=one, y=one):
        n = H * W
        xc = n if xc is None else xc
        rcs = n if rcs is None else rcs
        yc = n if yc is None else yc
        xb = Cmid * xc if xb is None else xb
        rb = C * rcs if rb is None else rb
        yb = C * yc if yb is None else yb
        return (x, gate, w_l, scale, shift, res, y, B, Cmid, C, H, W, xb, xc, rb, rcs, yb, yc, None)
    null_sweep(fn, ok(), (0, 1, 2, 5, 6), "project_fwd")
    assert fn(*ok(w_l=one + 4, scale=None, shift=None)) == -4
    for bad in (dict(B=0), dict(C=0), dict(Cmid=0), dict(H=-1), dict(W=0)):
        assert fn(*ok(**bad)) == -2, bad
    assert fn(*ok(xc=N - 1)) == -2 and b"overlap" in L.ts_last_error_string()
    assert fn(*ok(xb=96 * N - 1)) == -2 and fn(*ok(rcs=N - 1)) == -2 and fn(*ok(rb=24 * N - 1)) == -2
    assert fn(*ok(yc=N - 1)) == -2 and fn(*ok(yb=24 * N - 1)) == -2
    assert fn(*ok(C=513)) == -3 and fn(*ok(Cmid=2049)) == -3 and fn(*ok(C=512, Cmid=2048, x=None)) == -1
    assert fn(*ok(B=1, H=big, W=1)) == -3 and fn(*ok(B=1, H=1, W=big)) == -3
    assert fn(*ok(C=513, yc=N - 1, x=None)) == -2 and fn(*ok(C=513, x=None)) == -3
    # the overlap rules: y apart from x; the residual is y's own elements or apart from y
    assert fn(*ok(res=far, y=one)) == -2 and b"y overlaps x" in L.ts_last_error_string()              # an output over its own input
    assert fn(*ok(res=far, y=one + 4 * (2 * 96 * N - 1))) == -2 and b"y overlaps x" in L.ts_last_error_string()      # y begins on x's last element
    assert fn(*ok(res=far + 4, y=far)) == -2 and b"residual" in L.ts_last_error_string()              # a residual shifted against y
    assert fn(*ok(res=far, rcs=N + 1, y=far)) == -2 and b"residual" in L.ts_last_error_string()       # the same pointer, other strides
    # residual == y with equal strides is the in-place residual: it gets past the residual's rule, to the rule on x
    assert fn(*ok(x=far, res=far, y=far)) == -2 and b"y overlaps x" in L.ts_last_error_string()
    assert fn(*ok(res=far, y=one, w_l=one + 4)) == -4                                                 # after the alignment

    # ts_depthwise3x3_fwd(x, w, scale, shift, y, plane_sum, B, C, H, W, act, flip, x_bs, x_cs, y_bs, y_cs, stream)
    fn = L.ts_depthwise3x3_fwd

    def ok(B=2, C=12, H=9, W=13, act=1, flip=0, xb=None, xc=None, yb=None, yc=None, x=one, w=one, scale=one, shift=one, y=one, sums=one):
        n = H * W
        xc = n if xc is None else xc
        yc = n if yc is None else yc
        xb = C * xc if xb is None else xb
        yb = C * yc if yb is None else yb
        return (x, w, scale, shift, y, sums, B, C, H, W, act, flip, xb, xc, yb, yc, None)
    null_sweep(fn, ok(), (0, 1, 4), "depthwise3x3_fwd")
    for bad in (dict(B=0), dict(C=0), dict(H=0), dict(W=-3), dict(act=2), dict(act=-1), dict(flip=2), dict(flip=-1)):
        assert fn(*ok(**bad)) == -2, bad
    assert fn(*ok(xc=N - 1)) == -2 and b"overlap" in L.ts_last_error_string()
    assert fn(*ok(xb=12 * N - 1)) == -2 and fn(*ok(yc=N - 1)) == -2 and fn(*ok(yb=12 * N - 1)) == -2
    assert fn(*ok(B=1, H=big, W=1)) == -3 and fn(*ok(B=1, W=big, H=1)) == -3 and fn(*ok(B=1, C=big, H=1, W=1)) == -3 and fn(*ok(B=big, H=1, W=1)) == -3
    assert fn(*ok(B=1, H=big, x=None)) == -3 and fn(*ok(B=1, H=big, yc=1)) == -2
    # the overlap rule, after the pointers: y apart from x
    assert fn(*ok(y=one)) == -2 and b"y overlaps x" in L.ts_last_error_string()                       # an output over its own input
    assert fn(*ok(y=one + 4 * (2 * 12 * N - 1))) == -2 and b"overlaps" in L.ts_last_error_string()    # y begins on x's last element
    assert fn(*ok(y=one, w=None)) == -1

    # ts_depthwise3x3_bwd_weight(x, dy, dw, B, C, H, W, x_bs, x_cs, dy_bs, dy_cs, stream)
    fn = L.ts_depthwise3x3_bwd_weight
    ok = lambda B=2, C=12, H=9, W=13, xb=12 * N, xc=N, gb=12 * N, gc=N: (one, one, one, B, C, H, W, xb, xc, gb, gc, None)
    null_sweep(fn, ok(), (0, 1, 2), "depthwise3x3_bwd_weight")
    for bad in (dict(B=0), dict(C=-1), dict(H=0), dict(W=0)):
        assert fn(*ok(**bad)) == -2, bad
    assert fn(*ok(xc=N - 1)) == -2 and b"overlap" in L.ts_last_error_string()
    assert fn(*ok(xb=12 * N - 1)) == -2 and fn(*ok(gc=N - 1)) == -2 and fn(*ok(gb=12 * N - 1)) == -2
    assert fn(*ok(B=1, H=big, W=1, xc=big, gc=big)) == -3 and fn(*ok(B=1, C=big, H=1, W=1, xc=1, gc=1)) == -3

    # ts_se_gate_fwd(plane_sum, w_reduce, b_reduce, w_expand, b_expand, gate, B, Cmid, Cr, inv_hw, stream)
    fn = L.ts_se_gate_fwd
    ok = lambda B=2, Cmid=96, Cr=6: (one, one, one, one, one, one, B, Cmid, Cr, 0.25, None)
    null_sweep(fn, ok(), (0, 1, 2, 3, 4, 5), "se_gate_fwd")
    for bad in (dict(B=0), dict(Cmid=0), dict(Cr=-1)):
        assert fn(*ok(**bad)) == -2, bad
    assert fn(*ok(Cmid=2049)) == -3 and fn(*ok(Cr=513)) == -3 and fn(*ok(B=big)) == -3
    a = list(ok(Cmid=2048, Cr=512))
    a[5] = None
    assert fn(*a) == -1
