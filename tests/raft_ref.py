"""CorrBlock restated: the correlation pyramid and windowed lookup of RAFT-Stereo as the closed form the HIP kernels implement
(temporalstereo_amd/csrc/raft_corr.hip), in plain torch ops on any device, dtype following the inputs.  Pinned to the reference's
own runs by tests/test_raft_corr_cpu.py (fixtures tests/golden/raft_corr_*.npz); the expectation of tests/test_raft_corr_gpu.py
and the framework composition tools/raft_corr_bench.py times.

    P_0[b,y,x,x'] = sum_c fmap1[b,c,y,x] fmap2[b,c,y,x'] / sqrt(C)        sqrt(C) rounded to float32, as the reference's tensor is
    P_i           = mean of adjacent pairs of P_{i-1} along x' (an odd tail is dropped), W_i = W >> i
    out[b, i(2r+1)+k, y, x] = (1 - 2^-(i+1)) lerp0(P_i[b,y,x,:], xp),  xp = ((x - disp) / 2^i + (k - r)) W_i / (W - 1) - 0.5
lerp0: linear interpolation, zeros outside [0, W_i - 1].  `positions` takes the steps in the order the reference takes them."""
import os

import numpy as np
import torch

import synth


def corr_pyramid(fmap1, fmap2, num_levels):
    """[P_0, ..., P_{L-1}], P_i of shape [B, H, W, W >> i]."""
    C = fmap1.shape[1]
    scale = torch.sqrt(torch.tensor(C).float()).to(fmap1.dtype)
    level = torch.matmul(fmap1.permute(0, 2, 3, 1), fmap2.permute(0, 2, 1, 3)) / scale
    levels = [level]
    for _ in range(num_levels - 1):
        wi = level.shape[-1] // 2
        if wi < 1:
            raise ValueError("raft_ref: the level below is too narrow to pool")
        level = (level[..., 0:2 * wi:2] + level[..., 1:2 * wi:2]) / 2
        levels.append(level)
    return levels


def positions(disp, i, radius, Wi):
    """xp of level i for every pixel and tap, [B, H, W, 2r+1]: x - d, / 2^i, + (k - r), * 2 / (W - 1) - 1, ((. + 1) W_i - 1) / 2."""
    B, _, H, W = disp.shape
    x = torch.arange(W, device=disp.device, dtype=disp.dtype).view(1, 1, W, 1)
    delta = torch.arange(-radius, radius + 1, device=disp.device, dtype=disp.dtype).view(1, 1, 1, -1)
    t = (x - disp.permute(0, 2, 3, 1)) / 2 ** i
    g = 2 * (t + delta) / (W - 1) - 1
    return ((g + 1) * Wi - 1) / 2


def lookup(levels, disp, radius):
    """out [B, L(2r+1), H, W] from the levels of corr_pyramid."""
    outs = []
    for i, P in enumerate(levels):
        Wi = P.shape[-1]
        xp = positions(disp, i, radius, Wi)
        x0 = torch.floor(xp)
        w1 = xp - x0
        w0 = (x0 + 1) - xp
        i0 = x0.long()
        i1 = i0 + 1
        v0 = torch.gather(P, 3, i0.clamp(0, Wi - 1)) * ((i0 >= 0) & (i0 < Wi)).to(P.dtype)
        v1 = torch.gather(P, 3, i1.clamp(0, Wi - 1)) * ((i1 >= 0) & (i1 < Wi)).to(P.dtype)
        wy = 1.0 - 0.5 ** (i + 1)
        outs.append(v0 * (w0 * wy) + v1 * (w1 * wy))
    return torch.cat(outs, dim=-1).permute(0, 3, 1, 2).contiguous()


def corr_block(fmap1, fmap2, disp, num_levels=4, radius=4):
    return lookup(corr_pyramid(fmap1, fmap2, num_levels), disp, radius)


def dot_bound(fmap1, fmap2):
    """A = max over the row pairs of sum_c |fmap1| |fmap2| / sqrt(C), in float64: the scale of a C-term dot product's rounding."""
    a, b = fmap1.double().abs(), fmap2.double().abs()
    return float((torch.matmul(a.permute(0, 2, 3, 1), b.permute(0, 2, 1, 3)) / a.shape[1] ** 0.5).max())


def fixture_features(seed, shape):
    """fmap1, fmap2 of a fixture: N(0,1) float32 arrays, a pure function of the fixture's stored seed and shape."""
    return synth.normal(seed, "raft_fmap1", tuple(shape)), synth.normal(seed, "raft_fmap2", tuple(shape))


def load_fixture(tag):
    """tests/golden/raft_corr_<tag>.npz as a dict of arrays, with the feature maps drawn again from the stored seed."""
    g = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "raft_corr_%s.npz" % tag)))
    g["fmap1"], g["fmap2"] = fixture_features(int(g["seed"]), [int(v) for v in g["shape"]])
    return g
