"""Plain-torch restatement of the encoder's memory MBConv block and of the walk over a stage, written from their semantics, in the dtype
of the input -- the fp64 yardstick of tests/test_mbconv_{cpu,gpu}.py and the loader of tests/golden/mbconv_*.npz -- and a stand-in for the
block the reference takes from timm (InvertedResidual of efficientnetv2_rw_s: timm is not part of the reference's checkout, so the
stand-in is this project's text, with the attribute set the reference's function uses).

  mc = int(C * memory_percent);  x = cat([memory if given else input[:, :mc], input[:, mc:]], 1)
  x = silu(bn1(conv_pw(x)))                                   1x1, C -> Cmid, no bias            stage `act1`
  x = silu(bn2(conv_dw(x)))                                   3x3 depthwise, stride 1, padding 1, no bias       stage `act2`
  g = sigmoid(conv_expand(silu(conv_reduce(mean_hw(x)))))     both 1x1 with bias, Cmid -> Cr -> Cmid            stage `gate` [B, Cmid]
  out = input + bn3(conv_pwl(x * g))                          1x1, Cmid -> C, no bias;  new memory = input[:, :mc]
A fixture is a stage nn.Sequential(nn.Sequential(block, ...)) run over its frames: the memories of a frame are the previous frame's.
"""
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODES = ("train", "eval")
STAGES = ("act1", "act2", "gate")
EPS = 1e-5
SAMPLE = 8192                     # arrays with more elements are stored at this many seeded flat positions
MEMORY_PERCENT = 0.25
#        tag: batch, C, Cmid, Cr, plane, blocks, frames, memory of the first frame: None | 'given' | 'slice' (of a wider tensor)
CASES = {"a": dict(B=2, C=24, Cmid=96, Cr=6, plane=(5, 7), blocks=1, frames=1, memory="given"),            # mc = 6
         "b": dict(B=2, C=40, Cmid=240, Cr=10, plane=(9, 13), blocks=1, frames=1, memory=None),            # the first frame
         "c": dict(B=1, C=136, Cmid=544, Cr=34, plane=(6, 10), blocks=1, frames=1, memory="slice"),        # mc = 34: a seam inside a chunk, K over several flushes
         "d": dict(B=2, C=32, Cmid=128, Cr=8, plane=(17, 30), blocks=2, frames=2, memory=None)}            # the workload's 1/32 plane, two blocks, two frames
TAGS = tuple(CASES)


def block_key_shapes(C, Cmid, Cr):
    """The state-dict keys of one block, in the module's order, with their shapes."""
    def bn(name, c):
        return [(name + ".weight", (c,)), (name + ".bias", (c,)), (name + ".running_mean", (c,)), (name + ".running_var", (c,)),
                (name + ".num_batches_tracked", ())]
    return [("conv_pw.weight", (Cmid, C, 1, 1))] + bn("bn1", Cmid) + [("conv_dw.weight", (Cmid, 1, 3, 3))] + bn("bn2", Cmid) + \
        [("se.conv_reduce.weight", (Cr, Cmid, 1, 1)), ("se.conv_reduce.bias", (Cr,)), ("se.conv_expand.weight", (Cmid, Cr, 1, 1)),
         ("se.conv_expand.bias", (Cmid,)), ("conv_pwl.weight", (C, Cmid, 1, 1))] + bn("bn3", C)


BLOCK_KEYS = tuple(k for k, _ in block_key_shapes(1, 1, 1))


def key_shapes(tag):
    """The keys of a case's stage, `0.<block>.<block key>`, with their shapes."""
    c = CASES[tag]
    return [("0.%d.%s" % (i, k), s) for i in range(c["blocks"]) for k, s in block_key_shapes(c["C"], c["Cmid"], c["Cr"])]


def param_keys(tag):
    return tuple(k for k, _ in key_shapes(tag) if "running_" not in k and "num_batches" not in k)


# ------------------------------------------------------------------------------------------------------------------ the stand-in
class StandInSE(nn.Module):
    def __init__(self, chs, se_chs):
        super().__init__()
        self.conv_reduce = nn.Conv2d(chs, se_chs, 1, bias=True)
        self.act1 = nn.SiLU(inplace=True)
        self.conv_expand = nn.Conv2d(se_chs, chs, 1, bias=True)
        self.gate = nn.Sigmoid()

    def forward(self, x):
        x_se = x.mean((2, 3), keepdim=True)
        return x * self.gate(self.conv_expand(self.act1(self.conv_reduce(x_se))))


class StandInBlock(nn.Module):
    """What the reference's function asks of the block: the nine submodules, has_residual and drop_path_rate."""

    def __init__(self, C, Cmid, Cr):
        super().__init__()
        self.conv_pw = nn.Conv2d(C, Cmid, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(Cmid)
        self.act1 = nn.SiLU(inplace=True)
        self.conv_dw = nn.Conv2d(Cmid, Cmid, 3, 1, 1, groups=Cmid, bias=False)
        self.bn2 = nn.BatchNorm2d(Cmid)
        self.act2 = nn.SiLU(inplace=True)
        self.se = StandInSE(Cmid, Cr)
        self.conv_pwl = nn.Conv2d(Cmid, C, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(C)
        self.has_residual = True
        self.drop_path_rate = 0.0

    def forward(self, x):
        y = self.act1(self.bn1(self.conv_pw(x)))
        y = self.act2(self.bn2(self.conv_dw(y)))
        return x + self.bn3(self.conv_pwl(self.se(y)))


def stand_in_stage(tag):
    c = CASES[tag]
    return nn.Sequential(nn.Sequential(*[StandInBlock(c["C"], c["Cmid"], c["Cr"]) for _ in range(c["blocks"])]))


# ------------------------------------------------------------------------------------------------------------------ the restatement
def _bn(x, state, name, training, momentum):
    stats = not training or momentum is not None
    return F.batch_norm(x, state[name + ".running_mean"] if stats else None, state[name + ".running_var"] if stats else None,
                        state[name + ".weight"], state[name + ".bias"], training, 0.0 if momentum is None else momentum, EPS)


def block(inp, memory, state, training, memory_percent=MEMORY_PERCENT, momentum=None, prefix=""):
    """One block -> (output, new memory, dict(act1, act2, gate)).  state: tensors under `prefix` + the block keys.  The running statistics
    are left alone unless `momentum` is given in train mode: then they move IN PLACE as the framework's module moves them."""
    s = {k: state[prefix + k] for k in BLOCK_KEYS if not k.endswith("num_batches_tracked")}
    mc = int(inp.shape[1] * memory_percent)
    if memory is not None and memory.shape[1] != mc:
        raise AssertionError("input shape: {}; memory shape: {}!".format(inp.shape, memory.shape))
    first = inp[:, :mc]
    x = torch.cat([first if memory is None else memory, inp[:, mc:]], 1)
    a1 = F.silu(_bn(F.conv2d(x, s["conv_pw.weight"]), s, "bn1", training, momentum))
    a2 = F.silu(_bn(F.conv2d(a1, s["conv_dw.weight"], None, 1, 1, 1, a1.shape[1]), s, "bn2", training, momentum))
    pooled = a2.mean((2, 3), keepdim=True)
    gate = torch.sigmoid(F.conv2d(F.silu(F.conv2d(pooled, s["se.conv_reduce.weight"], s["se.conv_reduce.bias"])),
                                  s["se.conv_expand.weight"], s["se.conv_expand.bias"]))
    y = _bn(F.conv2d(a2 * gate, s["conv_pwl.weight"]), s, "bn3", training, momentum)
    return inp + y, first, dict(act1=a1, act2=a2, gate=gate.flatten(1))


def stage(inp, memories, state, blocks, training, memory_percent=MEMORY_PERCENT, momentum=None):
    """The walk over a stage of `blocks` blocks -> (output, new memories, [stages of block 0, ...])."""
    out_memories, stages = [], []
    for i in range(blocks):
        m = memories[i] if memories is not None and len(memories) > 0 else None
        inp, m, st = block(inp, m, state, training, memory_percent, momentum, "0.%d." % i)
        out_memories.append(m)
        stages.append(st)
    return inp, out_memories, stages


def run(seed, tag, dtype, training, backward=True):
    """The fixture's whole computation in `dtype` and one mode: dict(f<frame>_out, f<frame>_b<block>_<stage>; grad_in_f<frame>,
    grad_memory when the first frame is given one, grad_<parameter key>, of the seeded cotangents of every frame's output)."""
    c = CASES[tag]
    state = fixture_state(seed, tag, dtype)
    for k in param_keys(tag):
        state[k].requires_grad_(backward)
    ins = fixture_inputs(seed, tag, dtype)
    memory = fixture_memory(seed, tag, dtype)
    for t in ins + ([memory] if memory is not None else []):
        t.requires_grad_(backward)
    memories = [memory] if memory is not None else None
    res, outs = {}, []
    for f, x in enumerate(ins):
        out, memories, stages = stage(x, memories, state, c["blocks"], training)
        outs.append(out)
        res["f%d_out" % f] = out.detach()
        for i, st in enumerate(stages):
            for k in STAGES:
                res["f%d_b%d_%s" % (f, i, k)] = st[k].detach()
    if backward:
        torch.autograd.backward(outs, fixture_cotangents(seed, tag, dtype))
        for f, x in enumerate(ins):
            res["grad_in_f%d" % f] = x.grad.detach()
        if memory is not None:
            res["grad_memory"] = memory.grad.detach()
        for k in param_keys(tag):
            res["grad_" + k] = state[k].grad.detach()
    return res


# ------------------------------------------------------------------------------------------------------------------ fixtures
def fixture_state(seed, tag, dtype=torch.float32):
    """Seeded state under the stage's keys, in order: convolution weights N(0,1) * 2 / sqrt(fan-in), convolution biases N(0, 0.1),
    BatchNorm weight U(0.5, 1.5), bias N(0, 0.1), running mean N(0, 0.1), running variance U(0.5, 1.5), num_batches_tracked 0."""
    out = {}
    for k, shape in key_shapes(tag):
        if k.endswith("num_batches_tracked"):
            out[k] = torch.zeros((), dtype=torch.long)
            continue
        if len(shape) == 4:
            v = synth.normal(seed, "mb/" + k, shape).astype(np.float64) * (2.0 / np.sqrt(float(shape[1] * shape[2] * shape[3])))
        elif k.endswith("running_var") or (k.endswith(".weight") and ".bn" in k):
            v = synth.uniform(seed, "mb/" + k, shape, 0.5, 1.5)
        else:
            v = synth.normal(seed, "mb/" + k, shape).astype(np.float64) * 0.1
        out[k] = torch.from_numpy(np.asarray(v).astype(np.float32)).to(dtype)
    return out


def block_state(state, i=0):
    """The keys of block i of a stage's state, without their prefix."""
    p = "0.%d." % i
    return {k[len(p):]: v for k, v in state.items() if k.startswith(p)}


def in_shape(tag):
    c = CASES[tag]
    return (c["B"], c["C"]) + c["plane"]


def fixture_inputs(seed, tag, dtype=torch.float32):
    """One N(0,1) input per frame."""
    return [torch.from_numpy(synth.normal(seed, "mb/in/%d" % f, in_shape(tag))).to(dtype) for f in range(CASES[tag]["frames"])]


def fixture_memory(seed, tag, dtype=torch.float32):
    """The memory handed to the first frame, N(0,1), or None."""
    c = CASES[tag]
    if c["memory"] is None:
        return None
    return torch.from_numpy(synth.normal(seed, "mb/memory", (c["B"], int(c["C"] * MEMORY_PERCENT)) + c["plane"])).to(dtype)


def cotangent(seed, name, shape, dtype=torch.float32):
    """k / 8 with k an integer in [-8, 8]: exact in every float format."""
    rs = synth._rs(seed, "mb/cot/" + name)
    return torch.from_numpy(rs.randint(-8, 9, size=tuple(shape)) / 8.0).to(dtype)


def fixture_cotangents(seed, tag, dtype=torch.float32):
    return [cotangent(seed, "f%d" % f, in_shape(tag), dtype) for f in range(CASES[tag]["frames"])]


def stored(name):
    """Whether a fixture holds the ARRAY `name` = '<mode>_<key>' or 'grad_<mode>_<key>' beside its deviation: train mode the outputs
    and the gradients of the inputs, the memory and the three convolution weights; eval mode the outputs and the stages `act2` and
    `gate` (`act1`, and train mode's stages, are upstream of what is stored; everything has its dev_ / max_ / rel_grad_)."""
    if name.startswith("grad_"):
        mode, key = name[5:].split("_", 1)
        return mode == "train" and (key.startswith("in_f") or key == "memory" or key.endswith(("conv_pw.weight", "conv_dw.weight", "conv_pwl.weight")))
    mode, key = name.split("_", 1)
    if key.endswith("_out"):
        return True
    return mode == "eval" and key.endswith(("act2", "gate"))


def sample_index(seed, n):
    """The stored flat positions of an array of n elements (None: all of it)."""
    if n <= SAMPLE:
        return None
    return np.sort(np.random.RandomState((int(seed) + n) % (2 ** 32)).choice(n, SAMPLE, replace=False))


def sample(t, seed):
    """What a fixture stores of `t`: the whole array, or its seeded flat positions."""
    idx = sample_index(seed, t.numel())
    return t.reshape(-1) if idx is None else t.reshape(-1)[torch.as_tensor(idx, dtype=torch.long)]


def load_fixture(tag):
    g = dict(np.load(os.path.join(GOLDEN, "mbconv_%s.npz" % tag)))
    g["seed"] = int(g["seed"])
    g["keys"] = [str(k) for k in g["keys"]]
    g["key_shapes"] = [tuple(int(v) for v in row if v >= 0) for row in g["key_shapes"]]
    return g
