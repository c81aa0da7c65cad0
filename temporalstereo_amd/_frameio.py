"""What preprocess.py and augment.py share: the checks of their tensor arguments and the parts of the batch dictionary that do not
depend on how the frames were made.  Private: the public names live in those two modules."""
import torch

from . import _lib

_U16 = getattr(torch, "uint16", None)


def _on_gpu(what, *tensors):
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not torch.is_tensor(t):
            raise TypeError("%s: expected a tensor, got %s" % (what, type(t).__name__))
        if not t.is_cuda:
            raise RuntimeError("temporalstereo_amd ops run on the GPU only (got a %s tensor of shape %s); "
                               "there is deliberately no CPU fallback" % (t.device, tuple(t.shape)))
        if dev is not None and t.device != dev:
            raise RuntimeError("%s: tensors on %s and %s" % (what, dev, t.device))
        dev = t.device
    if dev is not None and dev.index != torch.cuda.current_device():
        raise RuntimeError("%s: tensors on %s while the current device is cuda:%d" % (what, dev, torch.cuda.current_device()))
    return dev


def _frames(what, left, right, layout):
    """uint8 images, one or a batch, of one shape -> (left, right, B, Hs, Ws, batched)"""
    if layout not in ('HWC', 'CHW'):
        raise ValueError("layout must be 'HWC' or 'CHW' (got %r)" % (layout,))
    for t in (left, right):
        if t is None:
            continue
        if not torch.is_tensor(t):
            raise TypeError("%s: expected a uint8 tensor, got %s" % (what, type(t).__name__))
        if t.dtype != torch.uint8:
            raise TypeError("%s: frames must be uint8 (got %s of shape %s)" % (what, t.dtype, tuple(t.shape)))
        if t.dim() not in (3, 4):
            raise ValueError("%s: a frame is [H,W,3] / [B,H,W,3] (HWC) or [3,H,W] / [B,3,H,W] (CHW), got shape %s" % (what, tuple(t.shape)))
        if t.shape[-1 if layout == 'HWC' else -3] != 3:
            raise ValueError("%s: three channels expected in layout %s, got shape %s" % (what, layout, tuple(t.shape)))
        if t.numel() == 0:
            raise ValueError("%s: empty batch of shape %s" % (what, tuple(t.shape)))
    if right is not None and tuple(right.shape) != tuple(left.shape):
        raise ValueError("%s: left has shape %s, right %s" % (what, tuple(left.shape), tuple(right.shape)))
    _on_gpu(what, left, right)
    batched = left.dim() == 4
    B = left.shape[0] if batched else 1
    Hs, Ws = (left.shape[-3], left.shape[-2]) if layout == 'HWC' else (left.shape[-2], left.shape[-1])
    return _lib.contiguous(left), (None if right is None else _lib.contiguous(right)), B, Hs, Ws, batched


def _three(name, v):
    v = tuple(float(x) for x in v)
    if len(v) != 3:
        raise ValueError("%s must hold three numbers (got %d)" % (name, len(v)))
    return v


def _out_tensor(what, t, shape, dev):
    if t.dtype != torch.float32 or not t.is_cuda or t.device != dev:
        raise TypeError("%s: out must be fp32 on %s (got %s on %s)" % (what, dev, t.dtype, t.device))
    if tuple(t.shape) != shape:
        raise ValueError("%s: out has shape %s, %s expected" % (what, tuple(t.shape), shape))
    _, _, H, W = shape
    if t.stride(3) != 1 or t.stride(2) != W or t.stride(1) != H * W or (shape[0] > 1 and t.stride(0) < 3 * H * W):
        raise ValueError("%s: an image of out must be dense (strides %s of shape %s); only the batch stride is free" % (what, t.stride(), shape))
    return t.stride(0) if shape[0] > 1 else 3 * H * W


def _color_outputs(what, sides, B, H, W, color_hw, out, color, dev):
    """The output tensors of a frames call -> (res, aug_stride): res['color_aug_' + s] is out= (checked: fp32 [B,3,H,W], dense
    images, one batch stride for both eyes) or new, res['color_' + s] is new [B,3,*color_hw] when `color`."""
    aug_shape = (B, 3, H, W)
    if out is not None:
        outs = tuple(out) if isinstance(out, (tuple, list)) else (out,)
        if len(outs) != len(sides):
            raise ValueError("%s: %d out tensors for %d eyes" % (what, len(outs), len(sides)))
        strides = {_out_tensor(what, t, aug_shape, dev) for t in outs}
        if len(strides) != 1:
            raise ValueError("%s: the out tensors must share one batch stride (got %s)" % (what, sorted(strides)))
        aug_stride = strides.pop()
    else:
        outs = tuple(torch.empty(aug_shape, device=dev, dtype=torch.float32) for _ in sides)
        aug_stride = 3 * H * W
    res = {'color_aug_' + s: t for s, t in zip(sides, outs)}
    if color:
        for s in sides:
            res['color_' + s] = torch.empty((B, 3) + tuple(color_hw), device=dev, dtype=torch.float32)
    return res, aug_stride


def _u16_map(what, raw, scale):
    """A 16-bit disparity map [H,W] / [B,H,W] / [B,1,H,W] as uint16, int16 (reinterpreted) or int32 (low 16 bits, a cast on the
    device) -> (the contiguous 16-bit map, (B, H, W, batched))"""
    _on_gpu(what, raw)
    if raw.dtype == torch.int32:
        if _lib.recording():
            raise RuntimeError("%s: an int32 map needs a cast that a launch plan would not replay; hand over 16-bit storage" % what)
        raw = raw.to(torch.int16)
    elif raw.dtype != torch.int16 and (_U16 is None or raw.dtype != _U16):
        raise TypeError("%s: raw must be uint16, int16 (reinterpreted) or int32 (got %s of shape %s)" % (what, raw.dtype, tuple(raw.shape)))
    if raw.dim() not in (2, 3, 4) or (raw.dim() == 4 and raw.shape[1] != 1) or raw.numel() == 0:
        raise ValueError("%s: raw must be a non-empty [H,W], [B,H,W] or [B,1,H,W] map (got %s)" % (what, tuple(raw.shape)))
    if not float(scale) > 0:
        raise ValueError("%s: scale %r" % (what, scale))
    batched = raw.dim() > 2
    return _lib.contiguous(raw), ((raw.shape[0] if batched else 1,) + tuple(raw.shape[-2:]) + (batched,))


def _batch_dict(what, fr, K_norm, k_size, S, baseline, timestamp):
    """The batch dictionary around the frames `fr` (the result of a frames call with both eyes): the colour entries, the
    ('K', s) / ('inv_K', s) views of the pyramid at k_size for s < S, and 'baseline' [B,1,1,1] from a number or B device values."""
    from .preprocess import intrinsics_pyramid
    if fr['color_aug_l'].dim() == 3:
        fr = {k: v.unsqueeze(0) for k, v in fr.items()}
    B = fr['color_aug_l'].shape[0]
    dev = fr['color_aug_l'].device
    t = timestamp
    batch = {('color', t, 'l'): fr['color_l'], ('color', t, 'r'): fr['color_r'],
             ('color_aug', t, 'l'): fr['color_aug_l'], ('color_aug', t, 'r'): fr['color_aug_r']}
    _on_gpu(what, K_norm)
    kn = K_norm if K_norm.dim() == 3 else K_norm.unsqueeze(0)
    if kn.shape[0] not in (1, B):
        raise ValueError("%s: K_norm of shape %s for a batch of %d" % (what, tuple(K_norm.shape), B))
    K, inv = intrinsics_pyramid(kn, k_size, S)
    if K.shape[0] != B:
        K, inv = K.expand(B, S, 4, 4), inv.expand(B, S, 4, 4)
    for s in range(S):
        batch[('K', s)] = K[:, s]
        batch[('inv_K', s)] = inv[:, s]
    if torch.is_tensor(baseline):
        _on_gpu(what, baseline)
        if baseline.numel() != B:
            raise ValueError("%s: baseline of shape %s for a batch of %d" % (what, tuple(baseline.shape), B))
        batch['baseline'] = baseline.to(torch.float32).reshape(B, 1, 1, 1)
    else:
        batch['baseline'] = torch.full((B, 1, 1, 1), float(baseline), device=dev, dtype=torch.float32)
    return batch


def _gt_rows(what, disp_gt_raw, batch):
    """disp_gt_raw with a leading batch axis, which must be the batch's"""
    B = batch['baseline'].shape[0]
    g = disp_gt_raw if disp_gt_raw.dim() > 2 else disp_gt_raw.unsqueeze(0)
    if g.shape[0] != B:
        raise ValueError("%s: disp_gt_raw of shape %s for a batch of %d" % (what, tuple(disp_gt_raw.shape), B))
    return g
