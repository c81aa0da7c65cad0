"""MemoryInvertedResidual on the device (temporalstereo_amd.MemoryInvertedResidual / block_forward / functional.mbconv_eval /
functional.depthwise_conv3x3; csrc/mbconv.hip) against the reference's own runs recorded in tests/golden/mbconv_*.npz (tools/gen_golden.py
--only-mbconv) and against tests/mbconv_ref.py and plain torch in fp64 on the CPU.  u = 2^-24.

Bars, none taken from the code under test (the convention of tests/test_decoder_gpu.py; the factor 4 is argued in
tests/test_raft_corr_gpu.py):
  stages and outputs   |hip - fp64| <= max(4 x dev_stage, 16 u max |stage|), dev_stage = max |fp32 run - fp64 run| of the reference on the
                       CPU: the fixture's, and for the shapes without a fixture (the single entries, the range case) the same figure from
                       an fp32 and an fp64 run of the same torch statements inside the test.
  gradients            against fp64: relative L2 <= max(4 x rel_grad_key, 1e-6); against the stored fp32 gradients (at the stored
                       positions): that plus rel_grad_key (triangle inequality).
Each case prints error / bar; with TS_MBCONV_PARITY_FILE set the line is appended to that file (profiles/mbconv_parity.txt is made so).
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import mbconv_ref as R
import synth
from compare import Parity, dev as _dev, gpu, same_bits, stage_bar
import temporalstereo_amd as ts
from temporalstereo_amd import _lib
from temporalstereo_amd import functional as TF
from temporalstereo_amd import layers

pytestmark = pytest.mark.gpu

P = Parity("TS_MBCONV_PARITY_FILE")
check, check_rel, against_fp64 = P.check, P.check_rel, P.against_fp64
MP = R.MEMORY_PERCENT
PLANES = ((1, 1), (1, 5), (5, 1), (3, 70), (40, 3), (6, 8), (10, 72))      # the last two: rows staged in 16-byte pieces, one and two column tiles


def t32(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float32))


# ------------------------------------------------------------------------------------------------------------------ the module
@functools.lru_cache(maxsize=None)
def case(tag, mode):
    g = R.load_fixture(tag)
    with torch.enable_grad():                  # (a caller may stand inside torch.no_grad(); the restatement runs its backward)
        return dict(g=g, seed=g["seed"], r64=R.run(g["seed"], tag, torch.float64, mode == "train"))


def stage_for(tag, seed, training, scale=1.0):
    c = R.CASES[tag]
    net = nn.Sequential(nn.Sequential(*[ts.MemoryInvertedResidual(c["C"], mid_chs=c["Cmid"], se_chs=c["Cr"], memory_percent=MP)
                                        for _ in range(c["blocks"])]))
    state = R.fixture_state(seed, tag)
    if scale != 1.0:
        state = {k: v * scale if v.dim() == 4 else v for k, v in state.items()}
    net.load_state_dict(state, strict=True)
    return net.to(_dev()).train(training)


def device_memory(tag, seed):
    """The first frame's memory on the device: None, dense, or (case c) a channel slice of a wider tensor."""
    memory = R.fixture_memory(seed, tag)
    if memory is None:
        return None
    if R.CASES[tag]["memory"] == "slice":
        wide = torch.full((memory.shape[0], memory.shape[1] + 5) + tuple(memory.shape[2:]), float("nan"), device=_dev())
        wide[:, 2:2 + memory.shape[1]] = gpu(memory)
        view = wide[:, 2:2 + memory.shape[1]]
        assert view.data_ptr() != wide.data_ptr() and view.stride(0) != view.shape[1] * view.stride(1)
        return view
    return gpu(memory)


def device_run(tag, mode, backward=None, ins=None, memory="fixture", stages=False):
    """The stage on the fixture's inputs -> dict(f<frame>_out, [f<frame>_b<block>_<stage>], grad_*)"""
    c = case(tag, mode)
    seed, training = c["seed"], mode == "train"
    backward = training if backward is None else backward
    net = stage_for(tag, seed, training)
    own = ins is None
    if own:
        ins = [gpu(t).requires_grad_(backward) for t in R.fixture_inputs(seed, tag)]
    if memory == "fixture":
        memory = device_memory(tag, seed)
        if memory is not None and backward:
            memory = memory.requires_grad_(True)           # (case c: the slice itself is the leaf)
    memories = [memory] if memory is not None else None
    res, outs = {}, []
    for f, x in enumerate(ins):
        if stages:                                         # the walk by hand, to see inside the blocks
            new = []
            for i, blk in enumerate(net[0]):
                m = memories[i] if memories else None
                assert blk._route(x, m) == "kernels"
                x, m, st = blk._kernel_forward(x, m, int(x.shape[1] * MP), return_stages=True)
                new.append(m)
                for k in R.STAGES:
                    res["f%d_b%d_%s" % (f, i, k)] = st[k]
            out, memories = x, new
        else:
            out, memories, idx = ts.block_forward(net, x, MP, memories, 0)
            assert idx == R.CASES[tag]["blocks"]
        outs.append(out)
        res["f%d_out" % f] = out.detach()
    if backward:
        torch.autograd.backward(outs, [gpu(t) for t in R.fixture_cotangents(seed, tag)])
        if own:
            for f, x in enumerate(ins):
                res["grad_in_f%d" % f] = x.grad
        if memory is not None and memory.is_leaf:
            res["grad_memory"] = memory.grad
        for k, p in net.named_parameters():
            res["grad_" + k] = p.grad
    return res


def compare_forward(tag, mode, got):
    c = case(tag, mode)
    g, seed, r64 = c["g"], c["seed"], c["r64"]
    for k in [k for k in got if not k.startswith("grad_")]:
        name = "%s_%s" % (mode, k)
        bar = stage_bar(float(g["dev_" + name]), float(g["max_" + name]))
        check("mbconv_%s %s" % (tag, name), got[k], r64[k], bar)
        if name in g:
            check("mbconv_%s %s (stored fp32)" % (tag, name), R.sample(got[k].cpu(), seed), torch.from_numpy(g[name]), bar + float(g["dev_" + name]))


@pytest.mark.parametrize("tag", R.TAGS)
def test_fixture_in_eval_mode_every_stage(tag):
    with torch.no_grad():
        got = device_run(tag, "eval", stages=True)
    c = R.CASES[tag]
    assert set(got) == {k for k in case(tag, "eval")["r64"] if not k.startswith("grad_")} and len(got) == c["frames"] * (1 + 3 * c["blocks"])
    compare_forward(tag, "eval", got)


def test_eval_form_through_block_forward_over_two_frames():
    with torch.no_grad():
        got = device_run("d", "eval")
        by_hand = device_run("d", "eval", stages=True)
    assert set(got) == {"f0_out", "f1_out"}
    compare_forward("d", "eval", got)
    for k in got:
        assert same_bits(got[k], by_hand[k]), k


@pytest.mark.parametrize("tag", R.TAGS)
def test_fixture_in_train_mode(tag):
    c = case(tag, "train")
    g, seed, r64 = c["g"], c["seed"], c["r64"]
    got = device_run(tag, "train")
    compare_forward(tag, "train", got)
    grads = [k for k in r64 if k.startswith("grad_")]
    assert set(grads) == {k for k in got if k.startswith("grad_")}
    for k in grads:
        name = "grad_train_" + k[5:]
        have, w64, rel = got[k], r64[k], float(g["rel_" + name])
        assert have is not None and have.shape == w64.shape, k
        bar = max(4.0 * rel, 1e-6)
        check_rel("mbconv_%s %s" % (tag, name), have, w64, w64, bar)
        if name in g:
            check_rel("mbconv_%s %s (stored fp32)" % (tag, name), R.sample(have.cpu(), seed), torch.from_numpy(g[name]), R.sample(w64, seed), bar + rel)


@pytest.mark.parametrize("tag", R.TAGS)
def test_train_forwards_update_the_running_statistics(tag):
    """Two train-mode forwards of the first frame (with the fixture's memory where it has one) move running_mean / running_var
    (momentum 0.1, unbiased variance) and num_batches_tracked of every block as the restatement's; bars as for a stage, from the
    restatement's own fp32 and fp64 runs."""
    seed, blocks = case(tag, "train")["seed"], R.CASES[tag]["blocks"]
    x, memory = R.fixture_inputs(seed, tag)[0], R.fixture_memory(seed, tag)

    def ref(dt):
        state = R.fixture_state(seed, tag, dt)
        with torch.no_grad():
            for _ in range(2):
                R.stage(x.to(dt), [memory.to(dt)] if memory is not None else None, state, blocks, True, momentum=0.1)
        return state
    s64, s32, before = ref(torch.float64), ref(torch.float32), R.fixture_state(seed, tag)
    net = stage_for(tag, seed, True)
    xd, md = gpu(x), device_memory(tag, seed)
    memories = [md] if md is not None else None
    assert net[0][0]._route(xd, md) == "train"
    ts.block_forward(net, xd, MP, memories, 0)                  # with autograd
    with torch.no_grad():
        ts.block_forward(net, xd, MP, memories, 0)              # and once more without
    got = net.state_dict()
    for k, _ in R.key_shapes(tag):
        if k.endswith("num_batches_tracked"):
            assert int(got[k]) == 2, k
        elif "running_" in k:
            assert float((s64[k] - before[k].double()).abs().max()) > 1e-3, k
            check("mbconv_%s after two train forwards %s" % (tag, k), got[k], s64[k],
                  stage_bar(float((s32[k].double() - s64[k]).abs().max()), float(s64[k].abs().max())))


@pytest.mark.parametrize("mode", R.MODES)
def test_two_runs_give_the_same_bits(mode, monkeypatch):
    # train mode: the 1x1 convolutions and the BatchNorms are the framework's there; it is asked for its deterministic algorithms
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)

    def once():
        if mode == "eval":
            with torch.no_grad():
                return device_run("d", mode, stages=True)
        return device_run("d", mode)
    one, two = once(), once()
    assert set(one) == set(two) and len(one) >= 10
    for k in one:
        assert same_bits(one[k], two[k]), k


def test_batch_slices_equal_single_image_calls():
    """B = 2 through the eval form equals two B = 1 calls bit for bit: no sum depends on the batch or on the grid it makes."""
    tag = "c"
    seed = case(tag, "eval")["seed"]
    net = stage_for(tag, seed, False)
    blk = net[0][0]
    x = gpu(torch.cat([R.fixture_inputs(seed, tag)[0], R.fixture_inputs(seed + 1, tag)[0]]))
    memory = gpu(torch.cat([R.fixture_memory(seed, tag), R.fixture_memory(seed + 1, tag)]))
    with torch.no_grad():
        both, _, st = blk._kernel_forward(x, memory, memory.shape[1], return_stages=True)
        for b in range(2):
            one, _, st1 = blk._kernel_forward(x[b:b + 1], memory[b:b + 1], memory.shape[1], return_stages=True)
            assert same_bits(one, both[b:b + 1]), b
            for k in R.STAGES:
                assert same_bits(st1[k], st[k][b:b + 1]), (b, k)


def test_operands_read_in_place_and_output_written_into_a_slice():
    """input (also the residual) and memory as batch and channel slices of NaN-filled wider tensors, the output into a slice of a
    sentinel-filled one: the bits of the dense call, the guards untouched."""
    tag = "a"
    seed = case(tag, "eval")["seed"]
    blk = stage_for(tag, seed, False)[0][0]
    x, memory = gpu(R.fixture_inputs(seed, tag)[0]), gpu(R.fixture_memory(seed, tag))
    B, C, H, W = x.shape
    mc = memory.shape[1]
    args = lambda: (blk.conv_pw.weight, TF._bn_eval_fold(blk.bn1), blk.conv_dw.weight, TF._bn_eval_fold(blk.bn2), blk.se.conv_reduce.weight,
                    blk.se.conv_reduce.bias, blk.se.conv_expand.weight, blk.se.conv_expand.bias, blk.conv_pwl.weight, TF._bn_eval_fold(blk.bn3))
    with torch.no_grad():
        dense = TF.mbconv_eval(x, memory, *args())
        wide_x = torch.full((2 * B, C + 4, H, W), float("nan"), device=_dev())
        wide_x[B:, 3:3 + C] = x
        wide_m = torch.full((B + 1, mc + 3, H, W), float("nan"), device=_dev())
        wide_m[:B, 1:1 + mc] = memory
        sentinel = -12345.5
        wide_y = torch.full((2 * B, C + 5, H, W), sentinel, device=_dev())
        view = wide_y[B:, 2:2 + C]
        before_x, before_m = wide_x.clone(), wide_m.clone()
        got = TF.mbconv_eval(wide_x[B:, 3:3 + C], wide_m[:B, 1:1 + mc], *args(), out=view)
        torch.cuda.synchronize()
    assert got.data_ptr() == view.data_ptr() and same_bits(view, dense) and not bool((dense == sentinel).any())
    rest = wide_y.clone()
    rest[B:, 2:2 + C] = sentinel
    assert bool((rest == sentinel).all())
    assert same_bits(wide_x.nan_to_num(7.0), before_x.nan_to_num(7.0)) and same_bits(wide_m.nan_to_num(7.0), before_m.nan_to_num(7.0))
    compare_forward(tag, "eval", dict(f0_out=view))


def test_output_over_the_input_in_place_and_shifted():
    """B = 2, C = 16, Cmid = 64, Cr = 4 on a 5 x 7 plane.  `out` the input itself is the in-place residual -- an element of the input is
    read by the thread that overwrites it -- and has the bits of the out-of-place call; an `out` that is the input shifted by one
    channel overlaps the residual without being its own elements and is refused (ts_mbconv_project_fwd, TS_ERR_SHAPE)."""
    B, C, Cmid, Cr, H, W = 2, 16, 64, 4, 5, 7
    torch.manual_seed(7480)
    blk = ts.MemoryInvertedResidual(C, mid_chs=Cmid, se_chs=Cr).to(_dev()).eval()
    x = gpu(t32(synth.normal(7480, "x", (B, C, H, W))))
    memory = gpu(t32(synth.normal(7480, "m", (B, int(C * MP), H, W))))
    args = lambda: (blk.conv_pw.weight, TF._bn_eval_fold(blk.bn1), blk.conv_dw.weight, TF._bn_eval_fold(blk.bn2), blk.se.conv_reduce.weight,
                    blk.se.conv_reduce.bias, blk.se.conv_expand.weight, blk.se.conv_expand.bias, blk.conv_pwl.weight, TF._bn_eval_fold(blk.bn3))
    with torch.no_grad():
        dense = TF.mbconv_eval(x, memory, *args())
        inplace = x.clone()
        got = TF.mbconv_eval(inplace, memory, *args(), out=inplace)
        torch.cuda.synchronize()
        assert got.data_ptr() == inplace.data_ptr() and same_bits(inplace, dense) and not same_bits(dense, x)
        wide = torch.zeros((B, C + 1, H, W), device=_dev())
        wide[:, :C] = x
        with pytest.raises(RuntimeError, match="overlaps"):
            TF.mbconv_eval(wide[:, :C], memory, *args(), out=wide[:, 1:])
        torch.cuda.synchronize()
    assert same_bits(wide[:, :C], x) and not bool(wide[:, C].any())           # refused before the launch: nothing was written


def test_weights_scaled_by_1e3():
    """Every convolution weight times 1e3: the pre-activations reach the far ends of SiLU and of the sigmoid; everything stays finite and
    within the bars of the restatement's own fp32 run."""
    tag = "a"
    seed = case(tag, "eval")["seed"]
    x, memory = R.fixture_inputs(seed, tag)[0], R.fixture_memory(seed, tag)

    def ref(dt):
        state = {k: (v * 1e3 if v.dim() == 4 else v) for k, v in R.fixture_state(seed, tag, dt).items()}
        out, _, st = R.block(x.to(dt), memory.to(dt), state, False, prefix="0.0.")
        return dict(st, out=out)
    r64, r32 = ref(torch.float64), ref(torch.float32)
    blk = stage_for(tag, seed, False, scale=1e3)[0][0]
    with torch.no_grad():
        out, _, got = blk._kernel_forward(gpu(x), gpu(memory), memory.shape[1], return_stages=True)
    got["out"] = out
    assert float(r64["act1"].abs().max()) > 1e3 and float(r64["gate"].min()) < 1e-6 and float(r64["gate"].max()) > 1 - 1e-6
    for k in ("act1", "act2", "gate", "out"):
        assert bool(torch.isfinite(got[k]).all()), k
        check("mbconv_a, weights x 1e3, %s" % k, got[k], r64[k], stage_bar(float((r32[k].double() - r64[k]).abs().max()), float(r64[k].abs().max())))


# ------------------------------------------------------------------------------------------------------------------ the entries alone
def laid(weight):
    """ts_mbconv_weight_layout of a [Cout, Cin] weight on the device"""
    Cout, Cin = weight.shape
    w_l = torch.empty(_lib.lib().ts_mbconv_weight_bytes(Cin, Cout) // 4, device=_dev())
    _lib.check(_lib.lib().ts_mbconv_weight_layout(_lib.ptr(weight), _lib.ptr(w_l), Cin, Cout, None), "ts_mbconv_weight_layout")
    return w_l


@pytest.mark.parametrize("seam", (1, "C-1", None))
def test_expand_entry(seam):
    """B = 2, C = 40, Cmid = 50 (three row blocks and a ragged fourth) on 9 x 13 (two pixel tiles, the second ragged)."""
    B, C, Cmid, H, W = 2, 40, 50, 9, 13
    mc = C - 1 if seam == "C-1" else (seam or 10)
    seed = 7400 + mc
    x, mem = t32(synth.normal(seed, "x", (B, C, H, W))), t32(synth.normal(seed, "m", (B, mc, H, W)))
    w = t32(synth.normal(seed, "w", (Cmid, C)).astype(np.float64) * (2.0 / np.sqrt(C)))
    scale, shift = t32(synth.uniform(seed, "s", (Cmid,), 0.5, 1.5)), t32(synth.normal(seed, "b", (Cmid,), 0.1))
    y = torch.full((B, Cmid, H, W), float("nan"), device=_dev())
    xd, md = gpu(x), (gpu(mem) if seam is not None else None)
    w_l, sd, bd = laid(gpu(w)), gpu(scale), gpu(shift)                 # (held in names: a temporary's memory is free for the next one)
    rc = _lib.lib().ts_mbconv_expand_fwd(_lib.ptr(md), _lib.ptr(xd), _lib.ptr(w_l), _lib.ptr(sd), _lib.ptr(bd), _lib.ptr(y),
                                         B, C, mc, Cmid, H, W, mc * H * W, H * W, C * H * W, H * W, Cmid * H * W, H * W, None)
    _lib.check(rc, "ts_mbconv_expand_fwd")

    def want(x, mem, w, scale, shift):
        cat = x if seam is None else torch.cat([mem, x[:, mc:]], 1)
        return F.silu(F.conv2d(cat, w[:, :, None, None]) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1))
    against_fp64("expand, seam %s" % seam, y, want, (x, mem, w, scale, shift))


def test_project_entry_with_a_strided_residual():
    """B = 2, Cmid = 300 (ten chunks: one flush of the blocked sums is crossed, the last chunk ragged), C = 24, on 9 x 13; the residual
    and the output are channel slices of wider tensors; scale and shift absent in a second call."""
    B, Cmid, C, H, W = 2, 300, 24, 9, 13
    seed = 7450
    x, gate = t32(synth.normal(seed, "x", (B, Cmid, H, W))), t32(synth.uniform(seed, "g", (B, Cmid), 0.0, 1.0))
    w = t32(synth.normal(seed, "w", (C, Cmid)).astype(np.float64) * (2.0 / np.sqrt(Cmid)))
    scale, shift = t32(synth.uniform(seed, "s", (C,), 0.5, 1.5)), t32(synth.normal(seed, "b", (C,), 0.1))
    res = t32(synth.normal(seed, "r", (B, C, H, W)))
    wide_r = torch.full((B, C + 7, H, W), float("nan"), device=_dev())
    wide_r[:, 4:4 + C] = gpu(res)
    rv = wide_r[:, 4:4 + C]
    w_l, xd, gd, sd, bd = laid(gpu(w)), gpu(x), gpu(gate), gpu(scale), gpu(shift)
    for with_affine in (True, False):
        wide_y = torch.full((B, C + 3, H, W), -7.25, device=_dev())
        yv = wide_y[:, 1:1 + C]
        rc = _lib.lib().ts_mbconv_project_fwd(_lib.ptr(xd), _lib.ptr(gd), _lib.ptr(w_l), _lib.ptr(sd) if with_affine else None,
                                              _lib.ptr(bd) if with_affine else None, _lib.ptr(rv), _lib.ptr(yv), B, Cmid, C, H, W,
                                              Cmid * H * W, H * W, rv.stride(0), rv.stride(1), yv.stride(0), yv.stride(1), None)
        _lib.check(rc, "ts_mbconv_project_fwd")

        def want(x, gate, w, scale, shift, res):
            y = F.conv2d(x * gate[:, :, None, None], w[:, :, None, None])
            if with_affine:
                y = y * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
            return y + res
        against_fp64("project, strided residual, affine %s" % with_affine, yv, want, (x, gate, w, scale, shift, res))
        assert bool((wide_y[:, :1] == -7.25).all()) and bool((wide_y[:, 1 + C:] == -7.25).all())


def test_pointwise_bits_do_not_depend_on_the_batch_grouping():
    """Both pointwise kernels at every MT.  Thirty-two images on a 24 x 24 plane (nine pixel tiles, the last ragged), 300 input
    channels (ten chunks: one flush of the blocked sums is crossed, the last chunk ragged; expand's seam at 75, inside a chunk) and 130
    output rows (a ragged last row group at every MT).  The launch rule (csrc/conv_pw1.hpp launch_rule, at least 512 workgroups) sends
    the first n images to
        n = 32  <8> (288 tiles x 2 row groups)    n = 20  <4> (180 x 3)    n = 12  <2> (108 x 5)    n = 4  <1> (36 x 9)
    of expand_kernel and of project_kernel -- every instantiation there is, with the prefetch depths 1, 2 and 4 and one to four staged
    weight pieces per thread.  Observed in a kernel trace of this test (a run of its own): profiles/mbconv_grouping_kernel_trace.txt.
    Every grouping has the bits of the n = 32 call; the n = 4 result also meets the fp64 statement at the stage bar."""
    B, Cin, rows, H, W, mc = 32, 300, 130, 24, 24, 75
    seed = 7470
    L = _lib.lib()
    scale, shift = t32(synth.uniform(seed, "s", (rows,), 0.5, 1.5)), t32(synth.normal(seed, "b", (rows,), 0.1))
    sd, bd = gpu(scale), gpu(shift)
    w = t32(synth.normal(seed, "w", (rows, Cin)).astype(np.float64) * (2.0 / np.sqrt(Cin)))
    w_l = laid(gpu(w))
    x, mem = t32(synth.normal(seed, "x", (B, Cin, H, W))), t32(synth.normal(seed, "m", (B, mc, H, W)))
    gate, res = t32(synth.uniform(seed, "g", (B, Cin), 0.0, 1.0)), t32(synth.normal(seed, "r", (B, rows, H, W)))
    xd, md, gd, rd = gpu(x), gpu(mem), gpu(gate), gpu(res)
    N = H * W

    def expand(n):
        y = torch.full((n, rows, H, W), float("nan"), device=_dev())
        _lib.check(L.ts_mbconv_expand_fwd(_lib.ptr(md), _lib.ptr(xd), _lib.ptr(w_l), _lib.ptr(sd), _lib.ptr(bd), _lib.ptr(y), n, Cin, mc, rows, H, W,
                                          mc * N, N, Cin * N, N, rows * N, N, None), "ts_mbconv_expand_fwd")
        return y

    def project(n):
        y = torch.full((n, rows, H, W), float("nan"), device=_dev())
        _lib.check(L.ts_mbconv_project_fwd(_lib.ptr(xd), _lib.ptr(gd), _lib.ptr(w_l), _lib.ptr(sd), _lib.ptr(bd), _lib.ptr(rd), _lib.ptr(y), n, Cin,
                                           rows, H, W, Cin * N, N, rows * N, N, rows * N, N, None), "ts_mbconv_project_fwd")
        return y

    def want_expand(x, mem, w, scale, shift):
        return F.silu(F.conv2d(torch.cat([mem, x[:, mc:]], 1), w[:, :, None, None]) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1))

    def want_project(x, gate, w, scale, shift, res):
        return F.conv2d(x * gate[:, :, None, None], w[:, :, None, None]) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1) + res
    for name, call in (("expand", expand), ("project", project)):
        whole = call(B)
        for n in (20, 12, 4):
            got = call(n)
            assert same_bits(got, whole[:n]), "%s, first %d images" % (name, n)
        assert n == 4
        if name == "expand":
            against_fp64("grouping, expand, first 4 images", got, want_expand, (x[:4], mem[:4], w, scale, shift))
        else:
            against_fp64("grouping, project, first 4 images", got, want_project, (x[:4], gate[:4], w, scale, shift, res[:4]))


def depthwise_inputs(plane, B=2, C=5):
    H, W = plane
    seed = 7500 + 100 * H + W
    return (t32(synth.normal(seed, "x", (B, C, H, W))), t32(synth.normal(seed, "w", (C, 1, 3, 3)).astype(np.float64) * (2.0 / 3.0)),
            t32(synth.uniform(seed, "s", (C,), 0.5, 1.5)), t32(synth.normal(seed, "b", (C,), 0.1)), R.cotangent(seed, "dw", (B, C, H, W)))


def depthwise_call(x, w, scale, shift, act, flip, sums):
    B, C, H, W = x.shape
    y = torch.full((B, C, H, W), float("nan"), device=_dev())
    s = torch.full((B, C), float("nan"), device=_dev()) if sums else None
    rc = _lib.lib().ts_depthwise3x3_fwd(_lib.ptr(x), _lib.ptr(w), _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(y), _lib.ptr(s), B, C, H, W, act, flip,
                                        x.stride(0), x.stride(1), C * H * W, H * W, None)
    _lib.check(rc, "ts_depthwise3x3_fwd")
    return y, s


@pytest.mark.parametrize("plane", PLANES)
def test_depthwise_entry(plane):
    x, w, scale, shift, _ = depthwise_inputs(plane)
    C = x.shape[1]
    xd, wd = gpu(x), gpu(w)

    def full(x, w, scale, shift):
        return F.silu(F.conv2d(x, w, None, 1, 1, 1, C) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1))

    def bare(x, w):
        return F.conv2d(x, w, None, 1, 1, 1, C)
    y, s = depthwise_call(xd, wd, gpu(scale), gpu(shift), 1, 0, True)
    against_fp64("depthwise %dx%d, epilogue" % plane, y, full, (x, w, scale, shift))
    against_fp64("depthwise %dx%d, plane sum" % plane, s, lambda *a: full(*a).sum((2, 3)), (x, w, scale, shift))
    y2, none = depthwise_call(xd, wd, gpu(scale), gpu(shift), 1, 0, False)
    assert none is None and same_bits(y2, y)
    y, s = depthwise_call(xd, wd, None, None, 0, 0, True)
    against_fp64("depthwise %dx%d, bare" % plane, y, bare, (x, w))
    against_fp64("depthwise %dx%d, bare, plane sum" % plane, s, lambda *a: bare(*a).sum((2, 3)), (x, w))
    # the same planes read from a channel slice whose rows are not 16-byte aligned: the bits of the dense call
    wide = torch.full((x.shape[0], C + 2) + plane, float("nan"), device=_dev())
    wide = wide.flatten()[1:1 + x.shape[0] * (C + 1) * plane[0] * plane[1]].view(x.shape[0], C + 1, *plane)
    wide[:, 1:] = xd
    y3, s3 = depthwise_call(wide[:, 1:], wd, None, None, 0, 0, True)
    assert same_bits(y3, y) and same_bits(s3, s)


@pytest.mark.parametrize("plane", PLANES)
def test_depthwise_gradient_entries(plane):
    x, w, _, _, cot = depthwise_inputs(plane)
    B, C, H, W = x.shape

    def grads(dt):
        xx, ww = x.clone().to(dt).requires_grad_(True), w.clone().to(dt).requires_grad_(True)
        F.conv2d(xx, ww, None, 1, 1, 1, C).backward(cot.to(dt))
        return xx.grad, ww.grad
    (gx64, gw64), (gx32, gw32) = grads(torch.float64), grads(torch.float32)
    xd, wd, gd = gpu(x), gpu(w), gpu(cot)
    gx, _ = depthwise_call(gd, wd, None, None, 0, 1, False)                 # flipped taps over dy, no epilogue
    check_rel("depthwise %dx%d, input gradient" % plane, gx, gx64, gx64, max(4.0 * float((gx32.double() - gx64).norm() / gx64.norm()), 1e-6))
    gw = torch.full((C, 1, 3, 3), float("nan"), device=_dev())
    rc = _lib.lib().ts_depthwise3x3_bwd_weight(_lib.ptr(xd), _lib.ptr(gd), _lib.ptr(gw), B, C, H, W, C * H * W, H * W, C * H * W, H * W, None)
    _lib.check(rc, "ts_depthwise3x3_bwd_weight")
    if float(gw64.norm()) > 0:
        check_rel("depthwise %dx%d, weight gradient" % plane, gw, gw64, gw64, max(4.0 * float((gw32.double() - gw64).norm() / gw64.norm()), 1e-6))
    live = gw64 != 0                                                        # a 1-wide or 1-high plane has taps that meet padding alone
    assert bool((gw.cpu()[~live] == 0).all())


def test_plane_sum_bits_do_not_depend_on_batch_or_channels():
    H, W = 17, 30
    x, w = t32(synth.normal(7600, "x", (3, 6, H, W))), t32(synth.normal(7600, "w", (6, 1, 3, 3)))
    xd, wd = gpu(x), gpu(w)
    _, whole = depthwise_call(xd, wd, None, None, 1, 0, True)
    for b in range(3):
        for c in range(6):
            _, one = depthwise_call(xd[b:b + 1, c:c + 1].contiguous(), wd[c:c + 1].contiguous(), None, None, 1, 0, True)
            assert same_bits(one, whole[b:b + 1, c:c + 1]), (b, c)


@pytest.mark.parametrize("Cr", (1, 10))
def test_se_gate_entry(Cr):
    B, Cmid, HW = 3, 300, 35
    seed = 7700 + Cr
    sums = t32(synth.normal(seed, "s", (B, Cmid)).astype(np.float64) * HW)
    wr, br = t32(synth.normal(seed, "wr", (Cr, Cmid)).astype(np.float64) * (2.0 / np.sqrt(Cmid))), t32(synth.normal(seed, "br", (Cr,), 0.1))
    we, be = t32(synth.normal(seed, "we", (Cmid, Cr)).astype(np.float64) * (2.0 / np.sqrt(Cr))), t32(synth.normal(seed, "be", (Cmid,), 0.1))
    gate = torch.full((B, Cmid), float("nan"), device=_dev())
    held = [gpu(t) for t in (sums, wr, br, we, be)]
    rc = _lib.lib().ts_se_gate_fwd(*[_lib.ptr(t) for t in held], _lib.ptr(gate),
                                   B, Cmid, Cr, 1.0 / HW, None)
    _lib.check(rc, "ts_se_gate_fwd")
    against_fp64("se gate, Cr = %d" % Cr, gate, lambda s, wr, br, we, be: torch.sigmoid(F.linear(F.silu(F.linear(s / HW, wr, br)), we, be)),
                 (sums, wr, br, we, be))


@pytest.mark.parametrize("C", (1, 7, 130))
def test_depthwise_conv3x3_function(C):
    B, H, W = 2, 9, 13
    seed = 7800 + C
    x, w, b = t32(synth.normal(seed, "x", (B, C, H, W))), t32(synth.normal(seed, "w", (C, 1, 3, 3)).astype(np.float64) * (2.0 / 3.0)), t32(synth.normal(seed, "b", (C,), 0.1))
    cot = R.cotangent(seed, "fn", (B, C, H, W))

    def ref(dt):
        t = [v.clone().to(dt).requires_grad_(True) for v in (x, w, b)]             # (a clone: .to() of the same dtype is the tensor itself)
        y = F.conv2d(t[0], t[1], t[2], 1, 1, 1, C)
        y.backward(cot.to(dt))
        return [y.detach()] + [v.grad for v in t]
    r64, r32 = ref(torch.float64), ref(torch.float32)
    t = [gpu(v).requires_grad_(True) for v in (x, w, b)]
    y = ts.depthwise_conv3x3(*t)
    y.backward(gpu(cot))
    check("depthwise_conv3x3 C = %d out" % C, y.detach(), r64[0], stage_bar(float((r32[0].double() - r64[0]).abs().max()), float(r64[0].abs().max())))
    for name, have, w64, w32 in zip(("x", "weight", "bias"), [v.grad for v in t], r64[1:], r32[1:]):
        check_rel("depthwise_conv3x3 C = %d grad %s" % (C, name), have, w64, w64, max(4.0 * float((w32.double() - w64).norm() / w64.norm()), 1e-6))
    y2 = ts.depthwise_conv3x3(t[0].detach(), t[1].detach())                # no bias
    check("depthwise_conv3x3 C = %d out, no bias" % C, y2, r64[0] - b.double().view(1, -1, 1, 1),
          stage_bar(float((r32[0].double() - r64[0]).abs().max()), float(r64[0].abs().max())))


# ------------------------------------------------------------------------------------------------------------------ routing
def test_module_routing(monkeypatch):
    """set_conv_backend('torch'), fp64, CPU tensors and a width beyond the envelope reach _reference_forward; train mode (or a gradient
    asked for) reaches _train_forward; eval mode on fp32 GPU tensors under the 'hip' backend reaches the kernels."""
    calls = []
    M = ts.MemoryInvertedResidual
    for name in ("_reference_forward", "_train_forward", "_kernel_forward"):
        real = getattr(M, name)
        monkeypatch.setattr(M, name, lambda self, *a, real=real, name=name, **k: calls.append(name) or real(self, *a, **k))
    tag = "a"
    c = case(tag, "eval")
    x, memory = R.fixture_inputs(c["seed"], tag)[0], R.fixture_memory(c["seed"], tag)
    xd, md = gpu(x), gpu(memory)
    m = stage_for(tag, c["seed"], False)[0][0]
    g = c["g"]
    bar = stage_bar(float(g["dev_eval_f0_out"]), float(g["max_eval_f0_out"]))
    with torch.no_grad():
        m(xd, md)
        assert calls == ["_kernel_forward"]
        assert layers._CONV_BACKEND["name"] == "hip"
        layers.set_conv_backend("torch")
        try:
            got, _ = m(xd, md)
        finally:
            layers.set_conv_backend("hip")
        assert calls[1:] == ["_reference_forward"]
        check("routing backend 'torch' out", got, c["r64"]["f0_out"], bar)
        m.cpu()(x, memory)
        m.to(_dev())
        m.double()(xd.double(), md.double())
        m.float()
        assert calls[2:] == ["_reference_forward"] * 2
        wide = M(516, mid_chs=8, se_chs=2).to(_dev()).eval()
        wide(torch.randn(1, 516, 3, 3, device=_dev()))
        assert calls[4:] == ["_reference_forward"]
    got, _ = m(xd.clone().requires_grad_(True), md)                   # eval mode, a gradient asked for
    assert calls[5:] == ["_train_forward"] and got.requires_grad
    check("routing eval mode with a gradient, out", got.detach(), c["r64"]["f0_out"], bar)
    m.train()
    with torch.no_grad():
        m(xd, md)
    assert calls[6:] == ["_train_forward"]
    m.eval()
    m.bn2.train()                                                      # one BatchNorm in train mode is train mode
    with torch.no_grad():
        m(xd, md)
    assert calls[7:] == ["_train_forward"] and len(calls) == 8


def test_eval_block_is_four_launches():
    """Inside WeightLayouts and BNFolds contexts an eval block issues exactly four launches (the first call lays the weights out and folds
    the BatchNorms); a bare call adds two weight layouts and three folds."""
    tag = "a"
    c = case(tag, "eval")
    m = stage_for(tag, c["seed"], False)[0][0]
    xd, md = gpu(R.fixture_inputs(c["seed"], tag)[0]), gpu(R.fixture_memory(c["seed"], tag))
    four = ["ts_mbconv_expand_fwd", "ts_depthwise3x3_fwd", "ts_se_gate_fwd", "ts_mbconv_project_fwd"]
    with torch.no_grad():
        with TF.WeightLayouts(), TF.BNFolds():
            first, _ = m(xd, md)
            with _lib.Recorder() as rec:
                second, _ = m(xd, md)
            assert [name for name, _ in rec.log] == four
        with _lib.Recorder() as rec:
            bare, _ = m(xd, md)
        assert sorted(name for name, _ in rec.log) == sorted(four + ["ts_mbconv_weight_layout"] * 2 + ["ts_bn_fold_many"] * 3)
    assert same_bits(first, second) and same_bits(first, bare)
