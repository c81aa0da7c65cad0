"""Plain-torch restatement of ConvGRU (the gated recurrent cell), written from its semantics, in the dtype of its input -- the fp64
yardstick of tests/test_conv_gru_{cpu,gpu}.py and the loader of tests/golden/conv_gru_*.npz.

  z      = sigmoid(3x3 conv, padding 1, bias, of cat[h, x])          update gate
  r      = sigmoid(3x3 conv, padding 1, bias, of cat[h, x])          reset gate
  q      = tanh(3x3 conv, padding 1, bias, of cat[r * h, x])         candidate
  hidden = (1 - z) * h + z * q
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYS = ("convz.weight", "convz.bias", "convr.weight", "convr.bias", "convq.weight", "convq.bias")
STAGES = ("z", "r", "q", "out")
SAMPLE = 8192                     # arrays with more elements are stored at this many seeded flat positions


def conv_gru(h, x, state):
    """One step -> dict(z, r, q, out)."""
    both = torch.cat((h, x), dim=1)
    z = torch.sigmoid(F.conv2d(both, state["convz.weight"], state["convz.bias"], padding=1))
    r = torch.sigmoid(F.conv2d(both, state["convr.weight"], state["convr.bias"], padding=1))
    q = torch.tanh(F.conv2d(torch.cat((r * h, x), dim=1), state["convq.weight"], state["convq.bias"], padding=1))
    return dict(z=z, r=r, q=q, out=(1 - z) * h + z * q)


def chain(h, x, state, steps=3):
    """`steps` steps in which the output is the next step's hidden state and x stays the same."""
    for _ in range(steps):
        h = conv_gru(h, x, state)["out"]
    return h


def run(seed, shape, dtype, backward=True):
    """The fixture's whole computation in `dtype`: dict(z, r, q, out of one step; out3 of three chained steps; grad_h, grad_x,
    grad_<key> of out3's seeded cotangent)."""
    B, Ch, Cx, H, W = shape
    state = {k: v.requires_grad_(backward) for k, v in fixture_state(seed, Ch, Cx, dtype).items()}
    h, x = fixture_input(seed, shape, dtype)
    h.requires_grad_(backward)
    x.requires_grad_(backward)
    res = {k: v.detach() for k, v in conv_gru(h, x, state).items()}
    out3 = chain(h, x, state)
    res["out3"] = out3.detach()
    if backward:
        out3.backward(fixture_cotangent(seed, out3.shape, dtype))
        res["grad_h"], res["grad_x"] = h.grad.detach(), x.grad.detach()
        for k in KEYS:
            res["grad_" + k] = state[k].grad.detach()
    return res


# ------------------------------------------------------------------------------------------------------------------ fixtures
def fixture_state(seed, Ch, Cx, dtype=torch.float32):
    """Seeded parameters under the module's state-dict keys, in its order: convolution weights N(0,1) * 2 / sqrt(9 (Ch + Cx)) (gate
    pre-activations of standard deviation 1.2-1.75, so both gates reach both ends of their range), biases N(0, 0.5)."""
    out = {}
    for k in KEYS:
        if k.endswith("weight"):
            v = synth.normal(seed, "gru/" + k, (Ch, Ch + Cx, 3, 3)).astype(np.float64) * (2.0 / np.sqrt(9.0 * (Ch + Cx)))
        else:
            v = synth.normal(seed, "gru/" + k, (Ch,)).astype(np.float64) * 0.5
        out[k] = torch.from_numpy(v.astype(np.float32)).to(dtype)
    return out


def fixture_input(seed, shape, dtype=torch.float32):
    """(h, x): h = tanh(N(0,1)), what a hidden state looks like after a step; x = N(0,1)."""
    B, Ch, Cx, H, W = shape
    h = np.tanh(synth.normal(seed, "gru/h", (B, Ch, H, W)).astype(np.float64)).astype(np.float32)
    x = synth.normal(seed, "gru/x", (B, Cx, H, W))
    return torch.from_numpy(h).to(dtype), torch.from_numpy(x).to(dtype)


def fixture_cotangent(seed, shape, dtype=torch.float32):
    """k / 8 with k an integer in [-8, 8]: exact in every float format."""
    rs = np.random.RandomState(int(seed) % (2 ** 32))
    return torch.from_numpy(rs.randint(-8, 9, size=tuple(shape)) / 8.0).to(dtype)


def sample_index(seed, n):
    """The stored flat positions of an array of n elements (None: all of it)."""
    if n <= SAMPLE:
        return None
    return np.sort(np.random.RandomState((int(seed) + n) % (2 ** 32)).choice(n, SAMPLE, replace=False))


def sample(t, seed):
    """What a fixture stores of `t`: the whole array, or its seeded flat positions."""
    idx = sample_index(seed, t.numel())
    return t if idx is None else t.reshape(-1)[torch.as_tensor(idx, dtype=torch.long)]


def load_fixture(tag):
    g = dict(np.load(os.path.join(GOLDEN, "conv_gru_%s.npz" % tag)))
    g["shape"] = tuple(int(s) for s in g["shape"])
    g["seed"] = int(g["seed"])
    g["keys"] = [str(k) for k in g["keys"]]
    return g
