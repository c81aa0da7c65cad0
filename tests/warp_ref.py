"""Test infrastructure: the semantics of the 2-D inverse warp restated in torch, dtype-generic (fp32 or fp64, CPU or GPU).

What temporalstereo_amd.inverse_warp computes, written down independently of the kernels: the source coordinate of every pixel of
the motion map (disparity / flow / depth through the rigid projection), normalised with the motion map's size and sampled by
grid_sample(align_corners=True), which un-normalises with the image's size.  tests/test_inverse_warp_cpu.py pins it to the
reference-made fixtures (tests/golden/inverse_warp_*.npz); the GPU tests use it for fp64 expectations at shapes without a fixture
and, through autograd, for the gradients.
"""
import torch
import torch.nn.functional as F


def pixel_grid(B, H, W, like):
    """x and y of every pixel, each [B, H, W], in the dtype and on the device of `like`"""
    xs = torch.arange(W, device=like.device, dtype=like.dtype).view(1, 1, W).expand(B, H, W)
    ys = torch.arange(H, device=like.device, dtype=like.dtype).view(1, H, 1).expand(B, H, W)
    return xs, ys


def project(depth, K, inv_K, T, eps=1e-7):
    """depth [B,1,H,W] -> the five products of the rigid projection: the 3-D point of every pixel (its ray through inv_K times the
    depth), moved by T and projected by K (identity-padded to 4x4 when 3x3); pixel coordinates = x, y over (z + eps)."""
    B, _, H, W = depth.shape
    xs, ys = pixel_grid(B, H, W, depth)
    if inv_K is None:
        inv_K = torch.inverse(K[:, :3, :3])
    rays = torch.stack((xs, ys, torch.ones_like(xs)), 1).reshape(B, 3, H * W)
    pts = torch.matmul(inv_K[:, :3, :3], rays) * depth.reshape(B, 1, H * W)
    homo = torch.cat((pts, torch.ones_like(pts[:, :1])), 1)
    if K.shape[-1] == 3:
        K4 = torch.eye(4, device=depth.device, dtype=depth.dtype).repeat(B, 1, 1)
        K4[:, :3, :3] = K
    else:
        K4 = K
    cam = torch.matmul(torch.matmul(K4, T)[:, :3], homo)
    coord = (cam[:, :2] / (cam[:, 2:3] + eps)).reshape(B, 2, H, W)
    sx, sy = coord[:, 0:1], coord[:, 1:2]
    return {'homo_points_3d': homo,
            'triangular_depth': cam[:, 2].reshape(B, 1, H, W),
            'flow_mask': (sx >= 0) & (sx <= W - 1) & (sy >= 0) & (sy <= H - 1),
            'src_pixel_coord': coord,
            'optical_flow': coord - torch.stack((xs, ys), 1)}


def source_coords(motion, mode, K=None, inv_K=None, T=None, eps=1e-7):
    """(X, Y, side outputs): the source coordinate of every pixel in pixels of the motion map, each [B, H, W]"""
    B, C, H, W = motion.shape
    xs, ys = pixel_grid(B, H, W, motion)
    if mode == 'disparity':
        assert C == 1
        return xs + motion[:, 0], ys, {}
    if mode == 'flow':
        assert C == 2
        return xs + motion[:, 0], ys + motion[:, 1], {}
    if mode == 'depth':
        assert C == 1
        side = project(motion, K, inv_K, T, eps)
        return side['src_pixel_coord'][:, 0], side['src_pixel_coord'][:, 1], side
    raise TypeError(mode)


def positions(motion, mode, img_size, K=None, inv_K=None, T=None, eps=1e-7):
    """the un-padded sampling position (ix, iy) in pixels of the image, each [B, H, W]"""
    H, W = motion.shape[2:]
    Hi, Wi = img_size
    X, Y, _ = source_coords(motion, mode, K, inv_K, T, eps)
    gx, gy = 2 * X / (W - 1) - 1, 2 * Y / (H - 1) - 1
    return (gx + 1) / 2 * (Wi - 1), (gy + 1) / 2 * (Hi - 1)


def inverse_warp(img, motion, mode='disparity', K=None, inv_K=None, T=None, interpolate_mode='bilinear', padding_mode='zeros',
                 eps=1e-7):
    """-> (warped [B,C,H,W], side outputs: five entries in depth mode, else {})"""
    H, W = motion.shape[2:]
    X, Y, side = source_coords(motion, mode, K, inv_K, T, eps)
    grid = torch.stack((2 * X / (W - 1) - 1, 2 * Y / (H - 1) - 1), dim=3)
    return F.grid_sample(img, grid, mode=interpolate_mode, padding_mode=padding_mode, align_corners=True), side
