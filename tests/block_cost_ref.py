"""Test infrastructure: a plain restatement of the cost volume, tap by tap, in the dtype of its inputs.  No GPU in here.

Restates  architecture/modeling/aggregation/utils/block_cost.py:16-83  and  layers/inverse_warp_3d.py:4-58  of the reference without
grid_sample, avg_pool3d or interpolate (oracle/cost_volume.py keeps those, so that its rounding is the reference's):
  int path       integer shift with zeros, then -(L - T)^2;
  sampled path   source position, floor, fraction, two taps with zero weight outside [0, W-1];
  correlation    -sum over groups of 8 channels of (pooled L - pooled T)^2 of the unpooled, 2x2 and 4x4 floor-pooled volumes;
  expansion      align-corners bilinear back to (H, W), written per tap, so that a pooled axis of size 1 (H or W in 4..7) is explicit:
                 scale 0, both taps on cell 0, fraction 0.

The position has a dtype of its own.  pos_dtype=torch.float32 is the reference's own fp32 sequence, every step rounded,
    xs = x + (-d);  gx = xs / (W-1) * 2 - 1;  ix = ((gx + 1) / 2) * (W-1)
which ts::source_position (csrc/warp.hpp) promises to reproduce bit for bit.  On float64 inputs that gives the two references of
tests/test_block_cost_forms_gpu.py:
  exact   pos_dtype = float64: everything in float64;
  mixed   pos_dtype = float32: column and fraction from the fp32 position, values and all arithmetic after it in float64.  The
          position's W-proportional fp32 noise is gone from the comparison, and the column a gradient with respect to the disparity
          belongs to is the kernel's by construction, at and near integer positions too (d position / d disparity is -1 exactly).
Gradients are autograd of this file.
"""
import torch

GROUP = 8


def source_position(disp, W, pos_dtype):
    """[B, D, H, W] candidates -> the position each output pixel samples the right row at, every step in pos_dtype"""
    d = disp.to(pos_dtype)
    x = torch.arange(W, dtype=pos_dtype).view(1, 1, 1, W)
    xs = x + (-d)
    gx = (xs / (W - 1) * 2) - 1
    return ((gx + 1) / 2) * (W - 1)


def warp_taps(right, disp, pos_dtype=None):
    """right [B, C, H, W], disp [B, D, H, W] -> [B, C, D, H, W]: (1 - f) R[x0] + f R[x0 + 1], a tap outside the row weighing 0"""
    B, C, H, W = right.shape
    D = disp.shape[1]
    dt = right.dtype
    pos_dtype = pos_dtype or dt
    if pos_dtype == dt:
        pos = source_position(disp, W, dt)
    else:                                   # the value of the pos_dtype sequence, the derivative -1 of x - d
        pos = source_position(disp.detach(), W, pos_dtype).to(dt) + (disp.detach() - disp)
    fl = torch.floor(pos.detach())
    f = pos - fl
    x0 = fl.to(torch.int64)
    x1 = x0 + 1
    w0 = (1 - f) * ((x0 >= 0) & (x0 < W)).to(dt)
    w1 = f * ((x1 >= 0) & (x1 < W)).to(dt)
    vol = right.unsqueeze(2).expand(B, C, D, H, W)
    take = lambda xi: torch.gather(vol, 4, xi.clamp(0, W - 1).unsqueeze(1).expand(B, C, D, H, W))
    return w0.unsqueeze(1) * take(x0) + w1.unsqueeze(1) * take(x1)


def shift_taps(right, D):
    """right [B, C, H, W] -> [B, C, D, H, W]: T[d][x] = right[x - d], 0 for x < d"""
    B, C, H, W = right.shape
    xi = (torch.arange(W).view(1, 1, W) - torch.arange(D).view(D, 1, 1)).expand(D, H, W)
    vol = right.unsqueeze(2).expand(B, C, D, H, W)
    return torch.gather(vol, 4, xi.clamp(0, W - 1).expand(B, C, D, H, W)) * (xi >= 0).to(right.dtype)


def pool_floor(v, k):
    """[..., H, W] -> [..., H // k, W // k]: mean of the k x k taps of each whole block, the ragged rest dropped"""
    if k == 1:
        return v
    Hs, Ws = v.shape[-2] // k, v.shape[-1] // k
    taps = v[..., :Hs * k, :Ws * k].reshape(v.shape[:-2] + (Hs, k, Ws, k))
    return taps.sum((-3, -1)) / (k * k)


def _axis_taps(n_in, n_out, dt):
    """align-corners taps of one axis as a matrix [n_out, n_in]: per output index, 1 - l on cell i0 and l on cell i1 = i0 + 1 (i0
    itself on the last cell and on an axis of size 1, where l is 0)"""
    scale = torch.tensor(n_in - 1, dtype=dt) / (n_out - 1) if n_out > 1 else torch.tensor(0, dtype=dt)
    src = scale * torch.arange(n_out, dtype=dt)
    i0 = src.to(torch.int64).clamp(max=n_in - 1)
    i1 = i0 + (i0 < n_in - 1).to(torch.int64)
    lam = src - i0.to(dt)
    m = torch.zeros(n_out, n_in, dtype=dt)
    rows = torch.arange(n_out)
    m[rows, i0] = 1 - lam
    m[rows, i1] += lam
    return m


def expand_bilinear(g, H, W):
    """[..., Hs, Ws] -> [..., H, W], align_corners=True: along W, then along H, two taps per axis (every other entry of the tap
    matrices is an exact zero)"""
    Hs, Ws = g.shape[-2:]
    if (Hs, Ws) == (H, W):
        return g
    return _axis_taps(Hs, H, g.dtype) @ (g @ _axis_taps(Ws, W, g.dtype).t())


def group_blocks(ref5, tgt5, scales):
    """block_cost.py:66-78 -> list of `scales` tensors [B, C / 8, D, H, W]"""
    B, C, D, H, W = ref5.shape
    out = []
    for s in range(int(scales)):
        e = pool_floor(ref5, 2 ** s) - pool_floor(tgt5, 2 ** s)
        g = -(e * e).reshape(B, C // GROUP, GROUP, D, e.shape[-2], e.shape[-1]).sum(2)
        out.append(expand_bilinear(g, H, W))
    return out


def block_cost(left, right, disp, scales=3, pos_dtype=None, omit_ref=0):
    """disp an int: the int path, [B, C + scales C/8, D, H, W].  disp [B, D, H, W]: the sampled path, [B, 2C + scales C/8, D, H, W];
    omit_ref = 1 leaves the reference half out (ts_block_cost_sampled_warped_*), 2 both halves (ts_block_cost_sampled_corr_fwd)."""
    B, C, H, W = left.shape
    if C % GROUP:
        raise ValueError("channel count must be a multiple of 8")
    if isinstance(disp, int):
        ref = left.unsqueeze(2).expand(B, C, disp, H, W)
        tgt = shift_taps(right, disp)
        e = ref - tgt
        return torch.cat([-(e * e)] + group_blocks(ref, tgt, scales), 1)
    ref = left.unsqueeze(2).expand(B, C, disp.shape[1], H, W)
    tgt = warp_taps(right, disp, pos_dtype)
    return torch.cat(([ref] if omit_ref < 1 else []) + ([tgt] if omit_ref < 2 else []) + group_blocks(ref, tgt, scales), 1)
