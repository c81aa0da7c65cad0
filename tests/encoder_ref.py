"""Plain-torch restatement of the encoder's large planes -- the stem, the ConvBnAct members of the first stage, the fused-MBConv
(edge-residual) members of the second and third -- and of the whole backbone's forward, written from their semantics, in the dtype of the
input: the fp64 yardstick of tests/test_encoder_{cpu,gpu}.py and the loader of tests/golden/encoder_*.npz.  Also the stand-ins for the
blocks the reference takes from timm (ConvBnAct, EdgeResidual and InvertedResidual of efficientnetv2_rw_s: timm is not part of the
reference's checkout, so the stand-ins are this project's text, with the attribute sets timm 0.4.12 gives those blocks) and for the
backbone module that holds them, whose `_forward` / `forward` the fixture generator binds to the reference's own.

  ConvBnAct   y = silu(bn1(conv(x)));  y + x where has_residual                       3x3, padding 1, no bias
  edge        mid = silu(bn1(conv_exp(x)))   3x3, stride 1 | 2, padding 1             stage `mid`
              y = bn2(conv_pwl(mid))         1x1;  y + x where has_residual
  MBConv      without a residual: mbconv_ref.block's statements with a stride on the depthwise convolution and no memory;
              with one: mbconv_ref.block (the memory spliced into the first int(C * memory_percent) input channels)
  backbone    both eyes along the batch; stem; block0; block1..block4 through the stage walk; decoder_ref.decoder
"""
import os

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import decoder_ref
import mbconv_ref
import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODES = ("train", "eval")
EPS = 1e-5
SAMPLE = 8192                     # arrays with more elements are stored at this many seeded flat positions
MEMORY_PERCENT = 0.25
# the miniature backbone of case d, in the form of temporalstereo_amd.backbone.ARCHS: a stem 3 -> 8, a ConvBnAct with skip, two fused
# stages (a stride-2 member and a residual one each), two MBConv stages (a non-residual stride-2 member and a residual one each)
MINI = dict(stem=8, se_ratio=0.25,
            stages=((("cn", 8, 1, 1.0, 1),), (("er", 12, 2, 4.0, 2),), (("er", 16, 2, 4.0, 2),), (("ir", 24, 2, 4.0, 2),), (("ir", 32, 2, 4.0, 2),)),
            out_channels=(0, 8, 12, 16, 20))
#        tag: what is run.  edge / stage: members (Cin, Cmid, Cout, stride) of ONE stage on `plane`; backbone: MINI on two frames
CASES = {"a": dict(kind="edge", B=2, members=((24, 96, 24, 1),), plane=(5, 7), frames=1),                     # residual
         "b": dict(kind="edge", B=2, members=((24, 96, 48, 2),), plane=(9, 13), frames=1),                    # stride 2, odd on both axes
         "c": dict(kind="stage", B=2, members=((12, 48, 24, 2), (24, 96, 24, 1)), plane=(17, 30), frames=1),  # through the stage walk
         "d": dict(kind="backbone", B=2, plane=(64, 96), frames=2)}
TAGS = tuple(CASES)
STEPS = ("stem", "block0", "block1", "block2", "block3", "block4")        # case d: what is recorded in front of the decoder
OUTS = ("x4", "x8", "x16")


def make_divisible(v, divisor=8):
    new = max(divisor, int(v + divisor / 2) // divisor * divisor)
    return new + divisor if new < 0.9 * v else new


# ------------------------------------------------------------------------------------------------------------------ the stand-ins
class StandInConvBnAct(nn.Module):
    def __init__(self, cin, cout, stride=1, skip=True):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(cout)
        self.act1 = nn.SiLU(inplace=True)
        self.has_residual = skip and stride == 1 and cin == cout
        self.drop_path_rate = 0.0

    def forward(self, x):
        shortcut = x
        x = self.act1(self.bn1(self.conv(x)))
        if self.has_residual:
            x += shortcut
        return x


class StandInEdge(nn.Module):
    def __init__(self, cin, cmid, cout, stride):
        super().__init__()
        self.conv_exp = nn.Conv2d(cin, cmid, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(cmid)
        self.act1 = nn.SiLU(inplace=True)
        self.se = nn.Identity()
        self.conv_pwl = nn.Conv2d(cmid, cout, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(cout)
        self.has_residual = cin == cout and stride == 1
        self.drop_path_rate = 0.0

    def forward(self, x):
        shortcut = x
        x = self.act1(self.bn1(self.conv_exp(x)))
        x = self.se(x)
        x = self.bn2(self.conv_pwl(x))
        if self.has_residual:
            x += shortcut
        return x


class StandInMB(nn.Module):
    """mbconv_ref.StandInBlock with a stride and an output width: has_residual only at stride 1 and equal widths."""

    def __init__(self, cin, cmid, cr, cout, stride):
        super().__init__()
        self.conv_pw = nn.Conv2d(cin, cmid, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(cmid)
        self.act1 = nn.SiLU(inplace=True)
        self.conv_dw = nn.Conv2d(cmid, cmid, 3, stride, 1, groups=cmid, bias=False)
        self.bn2 = nn.BatchNorm2d(cmid)
        self.act2 = nn.SiLU(inplace=True)
        self.se = mbconv_ref.StandInSE(cmid, cr)
        self.conv_pwl = nn.Conv2d(cmid, cout, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(cout)
        self.has_residual = cin == cout and stride == 1
        self.drop_path_rate = 0.0

    def forward(self, x):
        y = self.act1(self.bn1(self.conv_pw(x)))
        y = self.act2(self.bn2(self.conv_dw(y)))
        y = self.bn3(self.conv_pwl(self.se(y)))
        return x + y if self.has_residual else y


def members_of(table):
    """[[(kind, cin, cmid, cr, cout, stride), ...] per stage] of a table in the form of MINI."""
    width, out = table["stem"], []
    for runs in table["stages"]:
        stage = []
        for kind, cout, stride, exp, n in runs:
            for i in range(n):
                stage.append((kind, width, make_divisible(width * exp), make_divisible(width * table["se_ratio"], 1), cout, stride if i == 0 else 1))
                width = cout
        out.append(stage)
    return out


def stand_in_member(m):
    kind, cin, cmid, cr, cout, stride = m
    if kind == "cn":
        return StandInConvBnAct(cin, cout, stride)
    if kind == "er":
        return StandInEdge(cin, cmid, cout, stride)
    return StandInMB(cin, cmid, cr, cout, stride)


class StandInBackbone(nn.Module):
    """The attributes the reference's `_forward` / `forward` use, built from a table; `conv2d` is the wrapper class the decoder's
    submodules are made of (the reference's own Conv2d in the generator, temporalstereo_amd.layers.Conv2d in the tests).  It has no
    forward of its own: the generator calls the reference's functions with it as `self`."""

    def __init__(self, conv2d, table=MINI, memory_percent=MEMORY_PERCENT, norm="BN", activation="SiLU"):
        super().__init__()
        self.in_planes, self.memory_percent, self.norm, self.activation = 3, memory_percent, norm, activation
        self.conv_stem = nn.Conv2d(3, table["stem"], 3, 2, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(table["stem"])
        self.act1 = nn.SiLU(inplace=True)
        stages = members_of(table)
        for i, stage in enumerate(stages):
            setattr(self, "block%d" % i, nn.Sequential(nn.Sequential(*[stand_in_member(m) for m in stage])))
        c = [stage[-1][4] for stage in stages]
        o = table["out_channels"]

        def pair(cin, cout):
            return nn.Sequential(conv2d(cin, cout, 3, 1, 1, bias=False, norm=(norm, cout), activation=activation),
                                 conv2d(cout, cout, 3, 1, 1, bias=False, norm=None, activation=None))
        self.conv32 = conv2d(c[4], o[4], 3, 1, 1, bias=False, norm=None, activation=None)
        self.deconv32_16 = pair(o[4] + c[3], o[3])
        self.deconv16_8 = pair(o[3] + c[2], o[2])
        self.deconv8_4 = pair(o[2] + c[1], o[1])


def stand_in(tag, conv2d=None):
    """Cases a..c: the stage nn.Sequential(nn.Sequential(member, ...)); case d: the backbone."""
    c = CASES[tag]
    if c["kind"] == "backbone":
        return StandInBackbone(conv2d)
    return nn.Sequential(nn.Sequential(*[StandInEdge(*m) for m in c["members"]]))


def mini_channels():
    stages = members_of(MINI)
    return tuple(stage[-1][4] for stage in stages), MINI["out_channels"]


# ------------------------------------------------------------------------------------------------------------------ the restatement
def _bn(x, state, name, training, momentum):
    stats = not training or momentum is not None
    return F.batch_norm(x, state[name + ".running_mean"] if stats else None, state[name + ".running_var"] if stats else None,
                        state[name + ".weight"], state[name + ".bias"], training, 0.0 if momentum is None else momentum, EPS)


def conv_bn_act(x, state, p, stride, residual, training, momentum=None, conv="conv"):
    y = F.silu(_bn(F.conv2d(x, state[p + conv + ".weight"], None, stride, 1), state, p + "bn1", training, momentum))
    return y + x if residual else y


def edge(x, state, p, stride, residual, training, momentum=None):
    """-> (output, mid)"""
    mid = conv_bn_act(x, state, p, stride, False, training, momentum, conv="conv_exp")
    y = _bn(F.conv2d(mid, state[p + "conv_pwl.weight"]), state, p + "bn2", training, momentum)
    return (y + x if residual else y), mid


def mb_plain(x, state, p, stride, training, momentum=None):
    a1 = F.silu(_bn(F.conv2d(x, state[p + "conv_pw.weight"]), state, p + "bn1", training, momentum))
    a2 = F.silu(_bn(F.conv2d(a1, state[p + "conv_dw.weight"], None, stride, 1, 1, a1.shape[1]), state, p + "bn2", training, momentum))
    pooled = a2.mean((2, 3), keepdim=True)
    gate = torch.sigmoid(F.conv2d(F.silu(F.conv2d(pooled, state[p + "se.conv_reduce.weight"], state[p + "se.conv_reduce.bias"])),
                                  state[p + "se.conv_expand.weight"], state[p + "se.conv_expand.bias"]))
    return _bn(F.conv2d(a2 * gate, state[p + "conv_pwl.weight"]), state, p + "bn3", training, momentum)


def walk(x, state, prefix, stage, memories, idx, training, memory_percent, momentum=None, record=None):
    """One stage -> (x, new memories, idx).  record: a dict that takes b<i>_mid / b<i>_out of the fused members."""
    out = []
    for i, (kind, cin, cmid, cr, cout, stride) in enumerate(stage):
        p = "%s%d." % (prefix, i)
        residual = cin == cout and stride == 1
        if kind == "cn":
            x = conv_bn_act(x, state, p, stride, residual, training, momentum)
        elif kind == "er":
            x, mid = edge(x, state, p, stride, residual, training, momentum)
            if record is not None:
                record["b%d_mid" % i], record["b%d_out" % i] = mid, x
        elif residual and memory_percent > 0:
            m = memories[idx] if memories is not None and len(memories) > 0 else None
            x, m, _ = mbconv_ref.block(x, m, state, training, memory_percent, momentum, p)
            out.append(m)
            idx += 1
        elif residual:
            x = x + mb_plain(x, state, p, stride, training, momentum)
        else:
            x = mb_plain(x, state, p, stride, training, momentum)
    return x, out, idx


def backbone(l_img, r_img, memories, state, training, memory_percent=MEMORY_PERCENT, momentum=None, table=MINI):
    """-> (dict(stem, block0..block4, x4, x8, x16) over both eyes along the batch, new memories)"""
    x = torch.cat([l_img, r_img], 0)
    res = {}
    x = res["stem"] = conv_bn_act(x, state, "", 2, False, training, momentum, conv="conv_stem")
    idx, out = 0, []
    for i, stage in enumerate(members_of(table)):
        x, new, idx = walk(x, state, "block%d.0." % i, stage, memories, idx, training, memory_percent if i > 0 else 0.0, momentum)
        out.extend(new)
        res["block%d" % i] = x
    dec = {k: v for k, v in state.items() if k.startswith(("conv32", "deconv"))}
    res.update(decoder_ref.decoder(res["block1"], res["block2"], res["block3"], res["block4"], dec, training, momentum))
    return res, out


def forward(tag, state, ins, training, momentum=None):
    """A case's forward over all its frames -> (dict of every recorded stage and output, the tensors the cotangents belong to).
    momentum: the running statistics in `state` move in place (train mode), as the framework's modules move them."""
    c = CASES[tag]
    res, outs = {}, []
    if c["kind"] == "backbone":
        memories = []
        for f in range(c["frames"]):
            r, memories = backbone(ins[2 * f], ins[2 * f + 1], memories, state, training, momentum=momentum)
            for k, v in r.items():
                res["f%d_%s" % (f, k)] = v
            outs += [r[k] for k in OUTS]
    else:
        stage = [("er", m[0], m[1], 0, m[2], m[3]) for m in c["members"]]
        rec = {}
        out, memories, idx = walk(ins[0], state, "0.", stage, None, 0, training, MEMORY_PERCENT, momentum, record=rec)
        assert memories == [] and idx == 0
        for k, v in rec.items():
            res["f0_" + k] = v
        res["f0_out"] = out
        outs.append(out)
    return res, outs


def run(seed, tag, dtype, training, backward=True):
    """The fixture's whole computation in `dtype` and one mode.
    a, b, c: dict(f0_b<i>_mid, f0_b<i>_out, f0_out; grad_in_f0, grad_<parameter key>) of the seeded cotangent of the output.
    d: dict(f<frame>_<stem|block0..4|x4|x8|x16>; grad_l_f<frame>, grad_r_f<frame>, grad_<parameter key>) of the seeded cotangents of
    every frame's x4, x8 and x16; frame 1 reads frame 0's memories."""
    state = fixture_state(seed, tag, dtype)
    for k in param_keys(tag):
        state[k].requires_grad_(backward)
    ins = fixture_inputs(seed, tag, dtype)
    for t in ins:
        t.requires_grad_(backward)
    res, outs = forward(tag, state, ins, training)
    res = {k: v.detach() for k, v in res.items()}
    if backward:
        torch.autograd.backward(outs, fixture_cotangents(seed, tag, dtype))
        for name, x in zip(input_names(tag), ins):
            res["grad_" + name] = x.grad.detach()
        for k in param_keys(tag):
            res["grad_" + k] = state[k].grad.detach()
    return res


# ------------------------------------------------------------------------------------------------------------------ fixtures
def _plain_conv2d(cin, cout, k, s, p, bias=False, norm=None, activation=None):
    """The shape of a decoder wrapper's state: the convolution, and `norm` as a BatchNorm child where it has one."""
    conv = nn.Conv2d(cin, cout, k, s, p, bias=bias)
    if norm is not None:
        conv.norm = nn.BatchNorm2d(cout)
    return conv


def key_shapes(tag):
    """The state-dict keys of a case's stand-in, in the module's order, with their shapes."""
    return [(k, tuple(v.shape)) for k, v in stand_in(tag, _plain_conv2d).state_dict().items()]


def param_keys(tag):
    return tuple(k for k, _ in key_shapes(tag) if "running_" not in k and "num_batches" not in k)


def fixture_state(seed, tag, dtype=torch.float32):
    """Seeded state under the stand-in's keys, in order: convolution weights N(0,1) * 2 / sqrt(fan-in) (case d: 1 / sqrt(fan-in)), convolution
    biases N(0, 0.1), BatchNorm weight U(0.5, 1.5), bias N(0, 0.1), running mean N(0, 0.1), running variance U(0.5, 1.5), num_batches_tracked 0."""
    out = {}
    gain = 1.0 if CASES[tag]["kind"] == "backbone" else 2.0         # (case d is some twenty layers deep: a gain of 2 a layer leaves fp32 nothing)
    for k, shape in key_shapes(tag):
        if k.endswith("num_batches_tracked"):
            out[k] = torch.zeros((), dtype=torch.long)
            continue
        if len(shape) == 4:
            v = synth.normal(seed, "enc/" + k, shape).astype(np.float64) * (gain / np.sqrt(float(shape[1] * shape[2] * shape[3])))
        elif k.endswith("running_var") or (k.endswith(".weight") and (".bn" in k or k.startswith("bn") or ".norm." in k)):
            v = synth.uniform(seed, "enc/" + k, shape, 0.5, 1.5)
        else:
            v = synth.normal(seed, "enc/" + k, shape).astype(np.float64) * 0.1
        out[k] = torch.from_numpy(np.asarray(v).astype(np.float32)).to(dtype)
    return out


def input_names(tag):
    c = CASES[tag]
    if c["kind"] == "backbone":
        return [n for f in range(c["frames"]) for n in ("l_f%d" % f, "r_f%d" % f)]
    return ["in_f0"]


def in_shape(tag):
    c = CASES[tag]
    return (c["B"], 3 if c["kind"] == "backbone" else c["members"][0][0]) + c["plane"]


def out_shapes(tag):
    """The shapes of what the cotangents are drawn for, in order."""
    c = CASES[tag]
    H, W = c["plane"]
    if c["kind"] == "backbone":
        o = MINI["out_channels"]
        return [(2 * c["B"], o[i + 1], H >> (i + 2), W >> (i + 2)) for _ in range(c["frames"]) for i in range(3)]
    for m in c["members"]:
        H, W = (H + m[3] - 1) // m[3], (W + m[3] - 1) // m[3]
    return [(c["B"], c["members"][-1][2], H, W)]


def fixture_inputs(seed, tag, dtype=torch.float32):
    """N(0,1): the stage's input, or the left and right image of every frame."""
    return [torch.from_numpy(synth.normal(seed, "enc/" + n, in_shape(tag))).to(dtype) for n in input_names(tag)]


def cotangent(seed, name, shape, dtype=torch.float32):
    """k / 8 with k an integer in [-8, 8]: exact in every float format."""
    rs = synth._rs(seed, "enc/cot/" + name)
    return torch.from_numpy(rs.randint(-8, 9, size=tuple(shape)) / 8.0).to(dtype)


def fixture_cotangents(seed, tag, dtype=torch.float32):
    return [cotangent(seed, "o%d" % i, s, dtype) for i, s in enumerate(out_shapes(tag))]


def stored(name):
    """Whether a fixture holds the ARRAY `name` = '<mode>_<key>' or 'grad_<mode>_<key>' beside its deviation: the outputs (f<frame>_out, x4,
    x8, x16) in both modes, eval mode's mid maps, and train mode's gradients of the first input (case d: frame 0's left image) and of
    the 3x3 and 1x1 weights of the new blocks.  The rest would take the four files past 1 MB."""
    if name.startswith("grad_"):
        mode, key = name[5:].split("_", 1)
        return mode == "train" and (key in ("in_f0", "l_f0") or key.endswith(("conv_exp.weight", "conv_pwl.weight", "conv.weight", "conv_stem.weight")))
    mode, key = name.split("_", 1)
    if key.split("_", 1)[1] in ("out", "x4", "x8", "x16"):
        return True
    return mode == "eval" and key.endswith("_mid")


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
    g = dict(np.load(os.path.join(GOLDEN, "encoder_%s.npz" % tag)))
    g["seed"] = int(g["seed"])
    g["keys"] = [str(k) for k in g["keys"]]
    g["key_shapes"] = [tuple(int(v) for v in row if v >= 0) for row in g["key_shapes"]]
    return g
