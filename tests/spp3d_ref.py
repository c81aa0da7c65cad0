"""Plain-torch restatement of SPP3D (3-D pyramid pooling), written from its semantics, in the dtype of its input -- the fp64 yardstick
of tests/test_spp3d_{cpu,gpu}.py and the loader of tests/golden/spp3d_*.npz.

  level_s   = mean over non-overlapping boxes k = (min(D,s), min(H,s), min(W,s)); floor(n / k) cells per axis, the remainder dropped
  level_s   = ReLU(BatchNorm(1x1x1 conv C -> 16))
  level_s   = trilinear resize to (D, H, W), align_corners: position o * (n_in - 1) / (n_out - 1), a size-1 axis broadcasts
  out       = 1x1x1 conv(ReLU(BatchNorm(3x3x3 conv, padding 1, of cat[x, level_2, ...])))
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS, MOMENTUM, LEVEL_CHANNELS = 1e-5, 0.1, 16


def boxes(size, strides):
    return [tuple(min(n, s) for n in size) for s in strides]


def level_sizes(size, strides):
    return [tuple(n // k for n, k in zip(size, box)) for box in boxes(size, strides)]


def pool(x, strides):
    """[B,C,D,H,W] -> one [B,C,nd,nh,nw] per stride."""
    B, C = x.shape[:2]
    out = []
    for (kd, kh, kw), (nd, nh, nw) in zip(boxes(x.shape[2:], strides), level_sizes(x.shape[2:], strides)):
        v = x[:, :, :nd * kd, :nh * kh, :nw * kw].reshape(B, C, nd, kd, nh, kh, nw, kw)
        out.append(v.sum(dim=(3, 5, 7)) / (kd * kh * kw))
    return out


def _axis_taps(n_in, n_out, dtype):
    o = torch.arange(n_out, dtype=dtype)
    scale = torch.tensor(n_in - 1, dtype=dtype) / torch.tensor(max(n_out - 1, 1), dtype=dtype)      # formed in the run's own dtype
    pos = scale * o
    i0 = pos.floor().long().clamp_(max=n_in - 1)
    i1 = (i0 + 1).clamp_(max=n_in - 1)
    w1 = pos - i0.to(dtype)
    return i0, i1, 1 - w1, w1


def resize(level, size):
    """Trilinear, align_corners=True, one axis after the other (differentiable: gathers and products only)."""
    v = level
    for axis, n_out in zip((2, 3, 4), size):
        i0, i1, w0, w1 = _axis_taps(v.shape[axis], n_out, v.dtype)
        shape = [1] * 5
        shape[axis] = n_out
        v = v.index_select(axis, i0) * w0.view(shape) + v.index_select(axis, i1) * w1.view(shape)
    return v


def batchnorm(y, state, prefix, training):
    """-> (normalised, updated running statistics or None); biased variance for the normalisation, unbiased for the running one."""
    shape = (1, -1, 1, 1, 1)
    if training:
        n = y.numel() // y.shape[1]
        if n < 2:
            raise ValueError("Expected more than 1 value per channel when training, got input size %s" % (tuple(y.shape),))
        mean = y.mean(dim=(0, 2, 3, 4))
        var = ((y - mean.view(shape)) ** 2).mean(dim=(0, 2, 3, 4))
        new = {prefix + "running_mean": (1 - MOMENTUM) * state[prefix + "running_mean"] + MOMENTUM * mean.detach(),
               prefix + "running_var": (1 - MOMENTUM) * state[prefix + "running_var"] + MOMENTUM * var.detach() * n / (n - 1),
               prefix + "num_batches_tracked": state[prefix + "num_batches_tracked"] + 1}
    else:
        mean, var, new = state[prefix + "running_mean"], state[prefix + "running_var"], {}
    z = (y - mean.view(shape)) / torch.sqrt(var.view(shape) + EPS)
    return z * state[prefix + "weight"].view(shape) + state[prefix + "bias"].view(shape), new


def spp3d(x, state, strides, training):
    """-> dict(out, cat, pooled=[..], pre=[pre-activation of every ReLU: the L levels, then fuse.0], stats={updated buffers})."""
    B, C, D, H, W = x.shape
    pooled = pool(x, strides)
    feats, pre, stats = [x], [], {}
    for i, p in enumerate(pooled):
        y = torch.einsum("oc,bcdhw->bodhw", state["pools.%d.weight" % i].reshape(LEVEL_CHANNELS, C), p)
        z, new = batchnorm(y, state, "pools.%d.norm." % i, training)
        stats.update(new)
        pre.append(z)
        feats.append(resize(torch.relu(z), (D, H, W)))
    cat = torch.cat(feats, dim=1)
    z, new = batchnorm(F.conv3d(cat, state["fuse.0.weight"], None, 1, 1), state, "fuse.0.norm.", training)
    stats.update(new)
    pre.append(z)
    out = torch.einsum("oc,bcdhw->bodhw", state["fuse.1.weight"].reshape(C, C), torch.relu(z))
    return dict(out=out, cat=cat, pooled=pooled, pre=pre, stats=stats)


# ------------------------------------------------------------------------------------------------------------------ fixtures
def state_shapes(C, L):
    shapes = {}
    for i in range(L):
        shapes["pools.%d.weight" % i] = (LEVEL_CHANNELS, C, 1, 1, 1)
        for leaf, shp in (("weight", (LEVEL_CHANNELS,)), ("bias", (LEVEL_CHANNELS,)), ("running_mean", (LEVEL_CHANNELS,)),
                          ("running_var", (LEVEL_CHANNELS,)), ("num_batches_tracked", ())):
            shapes["pools.%d.norm.%s" % (i, leaf)] = shp
    shapes["fuse.0.weight"] = (C, C + LEVEL_CHANNELS * L, 3, 3, 3)
    for leaf, shp in (("weight", (C,)), ("bias", (C,)), ("running_mean", (C,)), ("running_var", (C,)), ("num_batches_tracked", ())):
        shapes["fuse.0.norm." + leaf] = shp
    shapes["fuse.1.weight"] = (C, C, 1, 1, 1)
    return shapes


def fixture_state(seed, C, L, dtype=torch.float32):
    """Seeded parameters and buffers under the module's state-dict keys (convolution weights a little larger than the initialiser's,
    so that every stage has outputs of order one).  A BatchNorm's bias is +-(1.5 .. 2.5) x its weight, sign per channel: a channel's ReLU
    is then mostly open or mostly shut, and of the ~10^5 pre-activations of a stage few lie near zero -- which is what lets a seed exist at
    which none lies within 32 fp32-vs-fp64 deviations of it (tools/gen_golden.py spp3d_cases).  Both kinds of channel occur."""
    vals = synth.state_values(state_shapes(C, L), seed)
    out = {}
    for k, v in vals.items():
        if k.endswith(".norm.bias"):
            sign = np.where(synth.uniform(seed, k + "/sign", v.shape) < 0.5, -1.0, 1.0)
            v = (sign * synth.uniform(seed, k + "/margin", v.shape, 1.5, 2.5) * vals[k[:-4] + "weight"]).astype(np.float32)
        t = torch.from_numpy(v)
        if k.endswith(".weight") and v.ndim == 5:
            t = t * 2.0
        out[k] = t if k.endswith("num_batches_tracked") else t.to(dtype)
    return out


def fixture_input(seed, shape, dtype=torch.float32):
    """N(0,1) noise plus, per (batch, channel), an offset and a ramp along every axis of order one: the means over the large boxes then
    differ at order one too.  (With noise alone the coarse cells are ~1/64 apart, and a BatchNorm over the two values a channel has at
    the coarsest level divides by that distance: it would amplify the fp32 rounding of the means by two orders of magnitude.)"""
    B, C = shape[:2]
    x = synth.normal(seed, "spp3d_x", tuple(shape)).astype(np.float64)
    x += synth.normal(seed, "spp3d_offset", (B, C, 1, 1, 1))
    for axis, n in zip((2, 3, 4), shape[2:]):
        if n > 1:
            view = [1] * 5
            view[axis] = n
            ramp = (np.arange(n, dtype=np.float64) / (n - 1) - 0.5).reshape(view)
            x += synth.uniform(seed, "spp3d_ramp%d" % axis, (B, C, 1, 1, 1), -2.0, 2.0) * 2.0 * ramp
    return torch.from_numpy(x.astype(np.float32)).to(dtype)


def fixture_cotangent(seed, shape, dtype=torch.float32):
    """k / 8 with k an integer in [-8, 8]: exact in every float format."""
    rs = np.random.RandomState(int(seed) % (2 ** 32))
    return torch.from_numpy(rs.randint(-8, 9, size=tuple(shape)) / 8.0).to(dtype)


def load_fixture(tag):
    g = dict(np.load(os.path.join(GOLDEN, "spp3d_%s.npz" % tag)))
    g["strides"] = tuple(int(s) for s in g["strides"])
    g["shape"] = tuple(int(s) for s in g["shape"])
    g["training"] = bool(g["training"])
    g["seed"] = int(g["seed"])
    return g


def sample(t, idx):
    """The stored positions of a large stage (cat_idx: flat indices into cat[:, C:])."""
    return t.reshape(-1)[torch.as_tensor(np.asarray(idx), dtype=torch.long)]
