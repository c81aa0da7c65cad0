"""Plain-torch restatement of the backbone's three-level decoder and of one of its fused layers, written from their semantics, in the
dtype of the input -- the fp64 yardstick of tests/test_decoder_{cpu,gpu}.py and the loader of tests/golden/decoder_*.npz.

  layer(up, skip)  = act(bn(conv3x3(cat([resize(up), skip], 1)) + bias)), the resize bilinear with align_corners=True to skip's plane,
                     the convolution with stride 1 and padding 1; up = None: the plain convolution of skip
  x32 = conv32(x32)
  x16 = deconv32_16.1(layer(x32, x16))     x8 = deconv16_8.1(layer(x16, x8))     x4 = deconv8_4.1(layer(x8, x4))
  the first convolution of each pair is followed by BatchNorm (batch statistics in train mode, running statistics in eval mode) and
  SiLU; no convolution has a bias.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CHANNELS = (24, 48, 64, 160, 272)
OUT_CHANNELS = (0, 64, 128, 256, 320)
PAIRS = ("deconv32_16", "deconv16_8", "deconv8_4")
OUTPUTS = ("x4", "x8", "x16")
INPUTS = ("x4", "x8", "x16", "x32")
MODES = ("train", "eval")
EPS = 1e-5
SAMPLE = 8192                     # arrays with more elements are stored at this many seeded flat positions
#             tag: batch, then the planes of x32, x16, x8, x4
GEOMETRIES = {"a": (2, (2, 3), (4, 6), (8, 12), (16, 24)),          # exact doublings
              "b": (2, (2, 4), (3, 7), (5, 13), (10, 25))}          # what a 40 x 100 image gives: no ratio is 2


def key_shapes(channels=CHANNELS, out_channels=OUT_CHANNELS):
    """The state-dict keys of the four submodules, in the module's order, with their shapes."""
    c, o = channels, out_channels
    out = [("conv32.weight", (o[4], c[4], 3, 3))]
    for name, cin, cout in (("deconv32_16", o[4] + c[3], o[3]), ("deconv16_8", o[3] + c[2], o[2]), ("deconv8_4", o[2] + c[1], o[1])):
        out += [(name + ".0.weight", (cout, cin, 3, 3)), (name + ".0.norm.weight", (cout,)), (name + ".0.norm.bias", (cout,)),
                (name + ".0.norm.running_mean", (cout,)), (name + ".0.norm.running_var", (cout,)),
                (name + ".0.norm.num_batches_tracked", ()), (name + ".1.weight", (cout, cout, 3, 3))]
    return out


KEYS = tuple(k for k, _ in key_shapes())
PARAM_KEYS = tuple(k for k in KEYS if "running_" not in k and "num_batches" not in k)


def resize(x, size):
    return F.interpolate(x, size=tuple(size), mode="bilinear", align_corners=True)


def fused_layer(up, skip, weight, bias=None, bn=None, activation=None, training=False, momentum=None):
    """One fused layer.  bn: dict(weight, bias, running_mean, running_var) or None.  The running statistics are left alone unless
    `momentum` is given in train mode: then they are updated IN PLACE as the framework's module does (unbiased variance)."""
    x = skip if up is None else (resize(up, skip.shape[-2:]) if skip is None else torch.cat([resize(up, skip.shape[-2:]), skip], 1))
    y = F.conv2d(x, weight, bias, stride=1, padding=1)
    if bn is not None:
        stats = not training or momentum is not None
        y = F.batch_norm(y, bn["running_mean"] if stats else None, bn["running_var"] if stats else None, bn["weight"], bn["bias"],
                         training, 0.0 if momentum is None else momentum, EPS)
    if activation == "SiLU":
        y = F.silu(y)
    elif activation is not None:
        raise ValueError(activation)
    return y


def decoder(x4, x8, x16, x32, state, training, momentum=None):
    """-> dict(x4, x8, x16), the module's three outputs.  momentum: see fused_layer (the running statistics in `state` move)."""
    up = fused_layer(None, x32, state["conv32.weight"])
    out = {}
    for name, key, skip in (("deconv32_16", "x16", x16), ("deconv16_8", "x8", x8), ("deconv8_4", "x4", x4)):
        bn = {k: state["%s.0.norm.%s" % (name, k)] for k in ("weight", "bias", "running_mean", "running_var")}
        up = fused_layer(None, fused_layer(up, skip, state[name + ".0.weight"], None, bn, "SiLU", training, momentum), state[name + ".1.weight"])
        out[key] = up
    return out


def run(seed, tag, dtype, training, backward=True):
    """The fixture's whole computation in `dtype` and one mode: dict(x4, x8, x16; grad_x4 .. grad_x32, grad_<parameter key> of the three
    outputs' seeded cotangents)."""
    state = fixture_state(seed, dtype)
    for k in PARAM_KEYS:
        state[k].requires_grad_(backward)
    maps = fixture_input(seed, tag, dtype)
    for t in maps.values():
        t.requires_grad_(backward)
    out = decoder(maps["x4"], maps["x8"], maps["x16"], maps["x32"], state, training)
    res = {k: v.detach() for k, v in out.items()}
    if backward:
        cots = fixture_cotangents(seed, tag, dtype)
        torch.autograd.backward([out[k] for k in OUTPUTS], [cots[k] for k in OUTPUTS])
        for k in INPUTS:
            res["grad_" + k] = maps[k].grad.detach()
        for k in PARAM_KEYS:
            res["grad_" + k] = state[k].grad.detach()
    return res


# ------------------------------------------------------------------------------------------------------------------ fixtures
def fixture_state(seed, dtype=torch.float32, channels=CHANNELS, out_channels=OUT_CHANNELS):
    """Seeded state under the module's keys, in its order: convolution weights N(0,1) * 2 / sqrt(9 Cin), BatchNorm weight U(0.5, 1.5),
    bias N(0, 0.1), running mean N(0, 0.1), running variance U(0.5, 1.5), num_batches_tracked 0."""
    out = {}
    for k, shape in key_shapes(channels, out_channels):
        if k.endswith("num_batches_tracked"):
            out[k] = torch.zeros((), dtype=torch.long)
            continue
        if len(shape) == 4:
            v = synth.normal(seed, "dec/" + k, shape).astype(np.float64) * (2.0 / np.sqrt(9.0 * shape[1]))
        elif k.endswith("running_var") or k.endswith("norm.weight"):
            v = synth.uniform(seed, "dec/" + k, shape, 0.5, 1.5)
        else:
            v = synth.normal(seed, "dec/" + k, shape).astype(np.float64) * 0.1
        out[k] = torch.from_numpy(np.asarray(v).astype(np.float32)).to(dtype)
    return out


def geometry_shapes(tag, channels=CHANNELS, out_channels=OUT_CHANNELS):
    """{x4, x8, x16, x32: input shape}, {x4, x8, x16: output shape}"""
    B, p32, p16, p8, p4 = GEOMETRIES[tag]
    ins = {"x4": (B, channels[1]) + p4, "x8": (B, channels[2]) + p8, "x16": (B, channels[3]) + p16, "x32": (B, channels[4]) + p32}
    outs = {"x4": (B, out_channels[1]) + p4, "x8": (B, out_channels[2]) + p8, "x16": (B, out_channels[3]) + p16}
    return ins, outs


def fixture_input(seed, tag, dtype=torch.float32):
    """The four maps, N(0,1)."""
    ins, _ = geometry_shapes(tag)
    return {k: torch.from_numpy(synth.normal(seed, "dec/in/" + k, s)).to(dtype) for k, s in ins.items()}


def cotangent(seed, name, shape, dtype=torch.float32):
    """k / 8 with k an integer in [-8, 8]: exact in every float format."""
    rs = synth._rs(seed, "dec/cot/" + name)
    return torch.from_numpy(rs.randint(-8, 9, size=tuple(shape)) / 8.0).to(dtype)


def fixture_cotangents(seed, tag, dtype=torch.float32):
    _, outs = geometry_shapes(tag)
    return {k: cotangent(seed, k, s, dtype) for k, s in outs.items()}


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
    g = dict(np.load(os.path.join(GOLDEN, "decoder_%s.npz" % tag)))
    g["seed"] = int(g["seed"])
    g["keys"] = [str(k) for k in g["keys"]]
    g["key_shapes"] = [tuple(int(v) for v in row if v >= 0) for row in g["key_shapes"]]
    return g
