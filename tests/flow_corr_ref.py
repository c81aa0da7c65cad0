"""FlowCorrBlock restated: the all-pairs correlation pyramid and windowed lookup of RAFT as the closed form the HIP kernels implement
(temporalstereo_amd/csrc/flow_corr.hip), in plain torch ops on any device, dtype following the inputs.  Pinned to the reference's
own runs by tests/test_flow_corr_cpu.py (fixtures tests/golden/flow_corr_*.npz); the expectation of tests/test_flow_corr_gpu.py
and the framework composition tools/flow_corr_bench.py times.

    N = H W; n, m number the pixels of fmap1, fmap2 row-major; S = sqrt(C) rounded to float32, as the reference's tensor is
    P_0[b,n,m] = (f1_n . f1_m - 2 f1_n . f2_m + f2_n . f2_m) / S          three full Gram matrices, the reference's arithmetic
    P_i[b,n]   = 2x2 mean of P_{i-1}[b,n] as an H_{i-1} x W_{i-1} image over m (an odd last row or column is dropped)
    out[b, i K^2 + a K + bb, y, x] = bilinear0(P_i[b,n], x_t / 2^i + (a - r), y_t / 2^i + (bb - r)),  (x_t, y_t) = coords[b,:,y,x]
bilinear0: bilinear interpolation, zeros outside; K = 2r + 1; the FIRST window index moves x.  `positions` takes the steps in the
order the reference takes them (normalise by D_i - 1, un-normalise as grid_sample with align_corners does)."""
import os

import numpy as np
import torch

import synth


def corr_pyramid(fmap1, fmap2, num_levels):
    """[P_0, ..., P_{L-1}], P_i of shape [B, H*W, H >> i, W >> i]."""
    B, C, H, W = fmap1.shape
    scale = torch.sqrt(torch.tensor(C).float()).to(fmap1.dtype)
    a, b = fmap1.reshape(B, C, H * W), fmap2.reshape(B, C, H * W)
    at, bt = a.transpose(1, 2), b.transpose(1, 2)
    level = ((torch.matmul(at, a) - 2 * torch.matmul(at, b) + torch.matmul(bt, b)) / scale).reshape(B, H * W, H, W)
    levels = [level]
    for _ in range(num_levels - 1):
        hi, wi = level.shape[-2] // 2, level.shape[-1] // 2
        if hi < 1 or wi < 1:
            raise ValueError("flow_corr_ref: the level below is too small to pool")
        level = (level[..., 0:2 * hi:2, 0:2 * wi:2] + level[..., 0:2 * hi:2, 1:2 * wi:2]
                 + level[..., 1:2 * hi:2, 0:2 * wi:2] + level[..., 1:2 * hi:2, 1:2 * wi:2]) / 4
        levels.append(level)
    return levels


def positions(coords, i, radius, Hi, Wi):
    """(xs, ys) of level i for every pixel and tap, each [B, H, W, 2r+1]: c / 2^i, + (k - r), * 2 / (D_i - 1) - 1, ((. + 1) / 2) (D_i - 1)."""
    delta = torch.arange(-radius, radius + 1, device=coords.device, dtype=coords.dtype).view(1, 1, 1, -1)
    res = []
    for ch, D in ((0, Wi), (1, Hi)):
        t = coords[:, ch].unsqueeze(-1) / 2 ** i + delta
        g = 2 * t / (D - 1) - 1
        res.append(((g + 1) / 2) * (D - 1))
    return res[0], res[1]


def lookup(levels, coords, radius):
    """out [B, L(2r+1)^2, H, W] from the levels of corr_pyramid."""
    B, _, H, W = coords.shape
    K = 2 * radius + 1
    outs = []
    for i, P in enumerate(levels):
        Hi, Wi = P.shape[-2:]
        flat = P.reshape(B, H * W, Hi * Wi)
        xs, ys = positions(coords, i, radius, Hi, Wi)
        xs, ys = xs.reshape(B, H * W, K, 1), ys.reshape(B, H * W, 1, K)          # [.., a, bb]: a moves x
        x0, y0 = torch.floor(xs), torch.floor(ys)
        wx = ((x0 + 1) - xs, xs - x0)
        wy = ((y0 + 1) - ys, ys - y0)
        acc = 0
        for dy in (0, 1):
            for dx in (0, 1):
                xi, yi = x0.long() + dx, y0.long() + dy
                inside = ((xi >= 0) & (xi < Wi) & (yi >= 0) & (yi < Hi)).to(P.dtype)
                idx = (yi.clamp(0, Hi - 1) * Wi + xi.clamp(0, Wi - 1)).reshape(B, H * W, K * K)
                v = torch.gather(flat, 2, idx).reshape(B, H * W, K, K)
                acc = acc + v * inside * (wx[dx] * wy[dy])
        outs.append(acc.reshape(B, H, W, K * K))
    return torch.cat(outs, dim=-1).permute(0, 3, 1, 2).contiguous()


def flow_corr_block(fmap1, fmap2, coords, num_levels=4, radius=4):
    return lookup(corr_pyramid(fmap1, fmap2, num_levels), coords, radius)


def dot_bound(fmap1, fmap2):
    """A = max over the pixel pairs of (sum |f1_n||f1_m| + 2 sum |f1_n||f2_m| + sum |f2_n||f2_m|) / sqrt(C), in float64: the scale
    of the rounding of a dot product of up to 2C terms, summed in any order."""
    B, C, H, W = fmap1.shape
    a, b = fmap1.double().abs().reshape(B, C, H * W), fmap2.double().abs().reshape(B, C, H * W)
    at, bt = a.transpose(1, 2), b.transpose(1, 2)
    return float(((torch.matmul(at, a) + 2 * torch.matmul(at, b) + torch.matmul(bt, b)) / C ** 0.5).max())


def fixture_features(seed, shape):
    """fmap1, fmap2 of a fixture: N(0,1) float32 arrays, a pure function of the fixture's stored seed and shape."""
    return synth.normal(seed, "flow_fmap1", tuple(shape)), synth.normal(seed, "flow_fmap2", tuple(shape))


def load_fixture(tag):
    """tests/golden/flow_corr_<tag>.npz as a dict of arrays, with the feature maps drawn again from the stored seed."""
    g = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "flow_corr_%s.npz" % tag)))
    g["fmap1"], g["fmap2"] = fixture_features(int(g["seed"]), [int(v) for v in g["shape"]])
    return g
