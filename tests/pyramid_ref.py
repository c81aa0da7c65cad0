"""Test infrastructure: the element stages of the aggregation pyramid (csrc/pyramid_ops.hip) restated in plain torch from the formulas
of the reference model the kernel comments cite -- not from the kernels.  CPU only.  Every function computes in the dtype of its
inputs: called on float64 it is the reference of tests/test_pyramid_ops_gpu.py, called on float32 it is the yardstick of
tests/pyramid_cases.py (the same formula in fp32).  tests/test_pyramid_ref_cpu.py pins it to the framework's own float64 ops.
"""
import torch
import torch.nn.functional as F

from test_upsamplers_autograd_gpu import _convex_ref as convex_upsample, _unet_ref as unet_upsample      # noqa: F401  (module.py:337-353, :468-482)


# ---- 5^3 pooling, stride 1, padding 2 (PyramidFusion, module.py:415-417) -----------------------------------------------------------
def _windows(x, value):
    """[B,C,D,H,W] -> [B,C,D,H,W,125]: every 5^3 window of x padded by 2 with `value`, taps in (d, y, x) order"""
    xp = F.pad(x, (2, 2, 2, 2, 2, 2), value=value)
    return xp.unfold(2, 5, 1).unfold(3, 5, 1).unfold(4, 5, 1).reshape(x.shape + (125,))


def pool5(x):
    """-> (avg_pool3d with count_include_pad, max_pool3d) for any D, H, W >= 1"""
    return _windows(x, 0.0).sum(-1) / 125, _windows(x, float("-inf")).amax(-1)


def pool5_argmax(x):
    """flat index (into D*H*W) of every window's maximum: the FIRST maximum in (d, y, x) order, found with a strict '>'"""
    B, C, D, H, W = x.shape
    win = _windows(x, float("-inf"))
    best = torch.full(x.shape, float("-inf"), dtype=x.dtype)
    tap = torch.full(x.shape, -1, dtype=torch.int64)
    for k in range(125):
        upd = win[..., k] > best
        best = torch.where(upd, win[..., k], best)
        tap = torch.where(upd, torch.full_like(tap, k), tap)
    assert int(tap.min()) >= 0
    d = torch.arange(D).view(D, 1, 1) + tap // 25 - 2
    y = torch.arange(H).view(1, H, 1) + (tap // 5) % 5 - 2
    xx = torch.arange(W).view(1, 1, W) + tap % 5 - 2
    return (d * H + y) * W + xx


def pool5_bwd(x, grad_avg, grad_max):
    """d/dx of pool5: the box filter of grad_avg / 125 (a symmetric kernel is its own adjoint) + grad_max added at each window's arg-max"""
    B, C = x.shape[:2]
    gx = pool5(grad_avg)[0].reshape(B, C, -1).clone()
    gx.scatter_add_(2, pool5_argmax(x).reshape(B, C, -1), grad_max.reshape(B, C, -1))
    return gx.reshape(x.shape)


# ---- past_conv + cat + sort + gather (coarse.py:84-105, fine.py:105-122) -----------------------------------------------------------
def silu(z):
    return z * torch.sigmoid(z)


def merge(vol, sample, mem_sample, mem_cost, w, scale, shift, K):
    """vol [B,C,D0,H,W]; sample [B,D0,H,W] or None (candidate i has disparity i); mem_sample / mem_cost [B,K,H,W] or None (zeros);
    w / scale / shift [C]: the memory candidates' volume is silu(w[c] * mem_cost * scale[c] + shift[c]) (Conv3d 1x1x1 without bias,
    BatchNorm as scale / shift, SiLU).  -> (sorted samples [B,D0+K,H,W], volume [B,C,D0+K,H,W] in that order, the order itself)"""
    B, C, D0, H, W = vol.shape
    dt = vol.dtype
    if sample is None:
        sample = torch.arange(D0, dtype=dt).view(1, D0, 1, 1).expand(B, D0, H, W)
    if K > 0:
        if mem_sample is None or mem_cost is None:
            mem_sample, mem_cost = torch.zeros(B, K, H, W, dtype=dt), torch.zeros(B, K, H, W, dtype=dt)
        v = lambda t: t.to(dt).view(1, C, 1, 1, 1)
        vol = torch.cat([vol, silu(v(w) * mem_cost.unsqueeze(1) * v(scale) + v(shift))], 2)
        sample = torch.cat([sample, mem_sample], 1)
    out_sample, order = torch.sort(sample, dim=1, stable=True)
    return out_sample, torch.gather(vol, 2, order.unsqueeze(1).expand(-1, C, -1, -1, -1)), order


def merge_bwd(sample, grad_out_vol, grad_out_sample):
    """the inverse permutation: grad_vol[:, :, order[r]] = grad_out_vol[:, :, r]; grad_out_sample None -> grad_sample zeros"""
    C = grad_out_vol.shape[1]
    order = torch.sort(sample, dim=1, stable=True)[1]
    gv = torch.zeros_like(grad_out_vol).scatter_(2, order.unsqueeze(1).expand(-1, C, -1, -1, -1), grad_out_vol)
    gs = torch.zeros_like(sample) if grad_out_sample is None else torch.zeros_like(sample).scatter_(1, order, grad_out_sample)
    return gv, gs


# ---- align_corners=True linear resizes ---------------------------------------------------------------------------------------------
def _axis(n_in, n_out, dtype):
    """source index of every destination index: dst * (in - 1) / (out - 1), 0 when out == 1 -> (i0, i1, weight of i1)"""
    scale = torch.tensor(n_in - 1, dtype=dtype) / torch.tensor(n_out - 1, dtype=dtype) if n_out > 1 else torch.tensor(0, dtype=dtype)
    s = torch.arange(n_out, dtype=dtype) * scale
    i0 = s.floor().long().clamp(max=n_in - 1)
    return i0, (i0 + 1).clamp(max=n_in - 1), s - i0.to(dtype)


def _lerp_axis(x, dim, n_out):
    i0, i1, w = _axis(x.shape[dim], n_out, x.dtype)
    shape = [1] * x.dim()
    shape[dim] = n_out
    w = w.view(shape)
    return x.index_select(dim, i0) * (1 - w) + x.index_select(dim, i1) * w


def resize_linear(x, size):
    """F.interpolate(x, size, 'bilinear' | 'trilinear', align_corners=True) over the last len(size) axes, written out (the 4 / 8 taps
    as a product of one-axis interpolations), so that a size-1 axis on either side is defined"""
    for i, n in enumerate(size):
        x = _lerp_axis(x, x.dim() - len(size) + i, n)
    return x


def resize3d_add_act(a, add, size, act):
    """ResidualBlock3D.forward (module.py:285-295): act(trilinear(a -> size) + add); add may be None; act 0 none, 1 SiLU"""
    v = resize_linear(a, size)
    if add is not None:
        v = v + add
    return silu(v) if act == 1 else v


def resize3d_add_act_bwd(a, add, grad_out, size, act):
    """-> (grad_a, grad_add) by autograd (grad_add of a missing add: the gradient of the pre-activation)"""
    a = a.clone().requires_grad_(True)
    add = (torch.zeros(a.shape[:2] + tuple(size), dtype=a.dtype) if add is None else add.clone()).requires_grad_(True)
    resize3d_add_act(a, add, size, act).backward(grad_out)
    return a.grad, add.grad


def resize_bilinear(x, size, value_scale=1.0):
    """F.interpolate(x * s, size, 'bilinear', align_corners=True) (coarse.py:91-96, precise.py:100-103)"""
    return resize_linear(x * value_scale, size)


def range_candidates(disp, r):
    """TemporalStereo.py:110,119 and fine.py:82-87: low = d - r, high = d + r, cand = |high - low| * {0, 3/8, 1/2, 5/8, 1} + min(low, high)
    disp [B,H,W] -> low, high [B,H,W], cand [B,5,H,W]"""
    low, high = disp - r, disp + r
    steps = torch.tensor([0.0, 0.375, 0.5, 0.625, 1.0], dtype=disp.dtype).view(1, 5, 1, 1)
    return low, high, (high - low).abs().unsqueeze(1) * steps + torch.minimum(low, high).unsqueeze(1)
