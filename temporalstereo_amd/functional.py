"""torch.autograd.Function wrappers over the C ABI (include/ts_hip.h).

Function-level drop-ins for the reference's hot-path ops:
  block_cost        architecture/modeling/aggregation/utils/block_cost.py:16
All ops require fp32 CUDA(HIP) tensors on an MI355X and raise otherwise: there is no CPU path.
"""
import torch

from . import _lib


def _stream():
    return _lib.current_stream_handle()


_QUERY = {}


def _q(name, *args):
    """A size query of the C ABI (pure function of its integer arguments), remembered: a training step asks ~1,300 of them."""
    key = (name,) + args
    v = _QUERY.get(key)
    if v is None:
        v = _QUERY[key] = int(getattr(_lib._real_lib(), name)(*args))
    return v


# Measurement hook (bench.py): when set, called as probe(key, launch) around the K1 C-ABI call so
# that HIP events can bracket exactly the library's launches on the launch stream.
_k1_probe = None


def _require_gpu(*tensors):
    """fp32 tensors of ONE GPU, and that GPU is the current device: the launch stream is the current device's
    current stream (`_stream`), so an op on tensors of another device would be enqueued on the wrong GPU's queue,
    unordered against the framework's work on theirs.  Callers on a non-current device wrap the call in
    `with torch.cuda.device_of(tensor):` (NativeAggregator / InferenceEngine do)."""
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("temporalstereo_amd ops run on the GPU only (got a %s tensor); "
                               "there is deliberately no CPU fallback" % t.device)
        if t.dtype != torch.float32:
            raise TypeError("temporalstereo_amd ops are fp32 (got %s)" % t.dtype)
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise RuntimeError("temporalstereo_amd op got tensors on different devices (%s and %s)" % (dev, t.device))
    if dev is not None and dev.index != torch.cuda.current_device():
        raise RuntimeError("temporalstereo_amd op on %s while the current device is cuda:%d: wrap the call in "
                           "`with torch.cuda.device_of(tensor):`" % (dev, torch.cuda.current_device()))


class _BlockCost(torch.autograd.Function):
    """K1.  forward: ts_block_cost_{int,sampled}_fwd; backward: ts_block_cost_{int,sampled}_bwd."""

    @staticmethod
    def forward(ctx, left, right, disp, num_disp, scales):
        _require_gpu(left, right, disp)
        if left.dim() != 4 or left.shape != right.shape:
            raise ValueError("reference_fm / target_fm must be [B,C,H,W] of equal shape")
        left = _lib.contiguous(left)
        right = _lib.contiguous(right)
        B, C, H, W = left.shape
        L = _lib.lib()
        sampled = disp is not None
        if sampled:
            if disp.dim() != 4 or disp.shape[0] != B or disp.shape[2:] != left.shape[2:]:
                raise ValueError("disp_sample must be [B,D,H,W] matching the feature maps")
            disp = _lib.contiguous(disp)
            D = disp.shape[1]
            ctot = 2 * C + scales * (C // 8)
        else:
            D = int(num_disp)
            ctot = C + scales * (C // 8)
        if C % 8 != 0:
            raise ValueError("channel count must be a multiple of 8 (block_cost.py:9)")
        out = torch.empty((B, ctot, D, H, W), device=left.device, dtype=torch.float32)
        ws = torch.empty(max(int(L.ts_block_cost_workspace_bytes(B, C, H, W, D, scales)), 256),
                         device=left.device, dtype=torch.uint8)
        def launch():
            if sampled:
                return L.ts_block_cost_sampled_fwd(_lib.ptr(left), _lib.ptr(right), _lib.ptr(disp), _lib.ptr(out),
                                                   _lib.ptr(ws), B, C, H, W, D, scales, _stream())
            return L.ts_block_cost_int_fwd(_lib.ptr(left), _lib.ptr(right), _lib.ptr(out), _lib.ptr(ws),
                                           B, C, H, W, D, scales, _stream())
        rc = launch() if _k1_probe is None else _k1_probe((B, C, H, W, D, sampled), launch)
        _lib.check(rc, "ts_block_cost_%s_fwd" % ("sampled" if sampled else "int"))
        ctx.save_for_backward(left, right, disp if sampled else None)
        ctx.meta = (B, C, H, W, D, scales, sampled)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        left, right, disp = ctx.saved_tensors
        B, C, H, W, D, scales, sampled = ctx.meta
        L = _lib.lib()
        grad_out = _lib.contiguous(grad_out)
        need_l, need_r, need_d = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        gl = torch.empty_like(left) if need_l else None
        gr = torch.empty_like(right) if need_r else None
        gd = torch.empty_like(disp) if (sampled and need_d) else None
        ws = torch.empty(max(int(L.ts_block_cost_bwd_workspace_bytes(B, C, H, W, D, scales)), 256),
                         device=left.device, dtype=torch.uint8)
        if sampled:
            rc = L.ts_block_cost_sampled_bwd(_lib.ptr(left), _lib.ptr(right), _lib.ptr(disp), _lib.ptr(grad_out),
                                             _lib.ptr(gl), _lib.ptr(gr), _lib.ptr(gd), _lib.ptr(ws),
                                             B, C, H, W, D, scales, _stream())
        else:
            rc = L.ts_block_cost_int_bwd(_lib.ptr(left), _lib.ptr(right), _lib.ptr(grad_out),
                                         _lib.ptr(gl), _lib.ptr(gr), _lib.ptr(ws),
                                         B, C, H, W, D, scales, _stream())
        _lib.check(rc, "ts_block_cost_%s_bwd" % ("sampled" if sampled else "int"))
        return gl, gr, gd, None, None


def _fms_args(reference_fm, target_fm, disp_sample):
    _require_gpu(reference_fm, target_fm, disp_sample)
    if reference_fm.dim() != 4 or reference_fm.shape != target_fm.shape:
        raise ValueError("reference_fm / target_fm must be [B,C,H,W] of equal shape")
    B, C, H, W = reference_fm.shape
    if disp_sample.dim() != 4 or disp_sample.shape[0] != B or disp_sample.shape[2:] != reference_fm.shape[2:]:
        raise ValueError("disp_sample must be [B,D,H,W] matching the feature maps")
    if C % 8 != 0:
        raise ValueError("the HIP kernels work on 8-channel groups: C=%d is not a multiple of 8" % C)
    return _lib.contiguous(reference_fm), _lib.contiguous(target_fm), _lib.contiguous(disp_sample), B, C, H, W, disp_sample.shape[1]


def _fms_backward(l, r, d, g_ref, g_warp, needs):
    """Gradients of [ref repeated | right warped by every candidate] w.r.t. (left, right, candidates): that volume is the
    first 2C channels of the sampled block cost, so its backward is ts_block_cost_sampled_bwd at scales = 1 with a zero
    gradient on the correlation planes (one padded copy of the incoming gradient; these ops are not on the shipped path)."""
    B, C, H, W = l.shape
    D = d.shape[1]
    L = _lib.lib()
    gpad = torch.zeros((B, 2 * C + C // 8, D, H, W), device=l.device, dtype=torch.float32)
    if g_ref is not None:
        gpad[:, :C] = g_ref
    gpad[:, C:2 * C] = g_warp
    gl = torch.empty_like(l) if needs[0] else None
    gr = torch.empty_like(r) if needs[1] else None
    gd = torch.empty_like(d) if needs[2] else None
    ws = torch.empty(max(int(L.ts_block_cost_bwd_workspace_bytes(B, C, H, W, D, 1)), 256), device=l.device, dtype=torch.uint8)
    rc = L.ts_block_cost_sampled_bwd(_lib.ptr(l), _lib.ptr(r), _lib.ptr(d), _lib.ptr(gpad), _lib.ptr(gl), _lib.ptr(gr), _lib.ptr(gd),
                                     _lib.ptr(ws), B, C, H, W, D, 1, _stream())
    _lib.check(rc, "ts_block_cost_sampled_bwd")
    return gl, gr, gd


class _CatFms(torch.autograd.Function):
    @staticmethod
    def forward(ctx, reference_fm, target_fm, disp_sample):
        l, r, d, B, C, H, W, D = _fms_args(reference_fm, target_fm, disp_sample)
        out = torch.empty((B, 2 * C, D, H, W), device=l.device, dtype=torch.float32)
        rc = _lib.lib().ts_cat_fms_fwd(_lib.ptr(l), _lib.ptr(r), _lib.ptr(d), _lib.ptr(out), B, C, H, W, D, _stream())
        _lib.check(rc, "ts_cat_fms_fwd")
        ctx.save_for_backward(l, r, d)
        return out

    @staticmethod
    def backward(ctx, g):
        l, r, d = ctx.saved_tensors
        C = l.shape[1]
        g = _lib.contiguous(g)
        return _fms_backward(l, r, d, g[:, :C], g[:, C:], ctx.needs_input_grad)


class _DifFms(torch.autograd.Function):
    @staticmethod
    def forward(ctx, reference_fm, target_fm, disp_sample):
        l, r, d, B, C, H, W, D = _fms_args(reference_fm, target_fm, disp_sample)
        out = torch.empty((B, C, D, H, W), device=l.device, dtype=torch.float32)
        ws = torch.empty(int(_lib.lib().ts_dif_fms_workspace_bytes()), device=l.device, dtype=torch.uint8)
        rc = _lib.lib().ts_dif_fms_fwd(_lib.ptr(l), _lib.ptr(r), _lib.ptr(d), _lib.ptr(out), _lib.ptr(ws), B, C, H, W, D, _stream())
        _lib.check(rc, "ts_dif_fms_fwd")
        ctx.save_for_backward(l, r, d)
        return out

    @staticmethod
    def backward(ctx, g):
        # dif_fms.py:33-41 differentiated by hand: |e| where the warped value is > 0, the tensor-wide maximum elsewhere
        # (torch.max() hands its gradient to the maximal element, split evenly among ties); the warp itself through
        # the cost-volume backward kernel
        l, r, d = ctx.saved_tensors
        B, C, H, W = l.shape
        with torch.no_grad():
            warped = _CatFms.apply(l, r, d)[:, C:]
            e = l.unsqueeze(2) - warped
            a = e.abs()
            keep = (warped > 0).to(g.dtype)
            g_a = g * keep
            g_max = (g * (1 - keep)).sum()
            top = (a == a.max()).to(g.dtype)
            g_a = g_a + top * (g_max / top.sum())
            g_e = g_a * torch.sign(e)
            gl, gr, gd = _fms_backward(l, r, d, None, -g_e, (False,) + tuple(ctx.needs_input_grad[1:]))
            gl = g_e.sum(2) if ctx.needs_input_grad[0] else None
        return gl, gr, gd


def cat_fms(reference_fm, target_fm, disp_sample):
    """aggregation/utils/cat_fms.py:5 (same arguments): [B,2C,D,H,W] = cat[left repeated over D, right warped by every
    candidate] (the shipped configs use block_cost).  Differentiable in all three arguments."""
    return _CatFms.apply(reference_fm, target_fm, disp_sample)


def dif_fms(reference_fm, target_fm, disp_sample):
    """aggregation/utils/dif_fms.py:5 (same arguments): [B,C,D,H,W] = |left - warped right| with the elements whose warped
    value is not > 0 filled with the tensor-wide maximum difference.  Differentiable in all three arguments."""
    return _DifFms.apply(reference_fm, target_fm, disp_sample)


class _InverseWarp3d(torch.autograd.Function):
    """img [B,C,H,W] (C % 8 == 0), disp [B,D,H,W] -> [B,C,D,H,W] sampled at x + disp (ts_inverse_warp_3d_fwd).  Backward: the warped
    half of ts_block_cost_sampled_bwd at scales = 1 (that op warps by -disp: the candidates go in negated, their gradient comes
    back negated)."""

    @staticmethod
    def forward(ctx, img, disp):
        B, C, H, W = img.shape
        D = disp.shape[1]
        out = torch.empty((B, C, D, H, W), device=img.device, dtype=torch.float32)
        rc = _lib.lib().ts_inverse_warp_3d_fwd(_lib.ptr(img), _lib.ptr(disp), _lib.ptr(out), B, C, H, W, D, _stream())
        _lib.check(rc, "ts_inverse_warp_3d_fwd")
        ctx.save_for_backward(img, disp)
        return out

    @staticmethod
    def backward(ctx, g):
        img, disp = ctx.saved_tensors
        _, gi, gd = _fms_backward(img, img, -disp, None, _lib.contiguous(g), (False, ctx.needs_input_grad[0], ctx.needs_input_grad[1]))
        return gi, (-gd if gd is not None else None)


def inverse_warp_3d(img, disp, padding_mode='zeros', disp_Y=None):
    """layers/inverse_warp_3d.py:4 (same arguments): img [B,C,H,W] or [B,C,D,H,W], disp [B,D,H,W] -> img sampled at x + disp,
    [B,C,D,H,W], zeros outside the row.  Differentiable in img and disp.  `padding_mode` other than 'zeros' and a `disp_Y` are not
    what any caller in the reference asks for (block_cost.py:56, cat_fms.py:31, dif_fms.py:31) and are refused; wrong ranks raise the
    reference's own ValueError (inverse_warp_3d.py:31-33)."""
    if img.dim() not in (4, 5):
        raise ValueError('image is only allowed with 4 or 5 dimensions, but got {} dimensions!'.format(img.dim()))
    if disp.dim() != 4:
        raise ValueError("disp must be [B, D, H, W]")
    if padding_mode != 'zeros' or disp_Y is not None:
        raise RuntimeError("inverse_warp_3d: padding_mode=%r / disp_Y are not supported by the HIP kernel (TS_ERR_UNSUPPORTED): the reference "
                           "only ever calls it with 'zeros' and no disp_Y" % (padding_mode,))
    _require_gpu(img, disp)
    B, D, H, W = disp.shape
    if img.dim() == 5:
        if img.shape[2] != D:
            raise AssertionError('The disparity number should be same between image and disparity map!')
        if img.stride(2) == 0 or D == 1:
            img = img[:, :, 0]                       # an expanded view (cat_fms.py:28-31): every plane is the same image
        else:
            # plane d is warped by candidate d: B * D images with one candidate each (the kernel wants two: the row is doubled)
            C = img.shape[1]
            flat = img.permute(0, 2, 1, 3, 4).reshape(B * D, C, img.shape[3], img.shape[4])
            dd = disp.reshape(B * D, 1, H, W).expand(B * D, 2, H, W)
            return inverse_warp_3d(flat, dd)[:, :, 0].reshape(B, D, C, H, W).permute(0, 2, 1, 3, 4)
    if img.shape[0] != B or img.shape[2:] != disp.shape[2:]:
        raise ValueError("img [B,C,H,W] and disp [B,D,H,W] must agree in B, H, W")
    C = img.shape[1]
    if D == 1:
        return inverse_warp_3d(img, disp.expand(B, 2, H, W))[:, :, :1]
    pad = (-C) % 8
    x = _lib.contiguous(img.float())
    if pad:
        x = torch.cat([x, x.new_zeros(B, pad, H, W)], 1)
    out = _InverseWarp3d.apply(x, _lib.contiguous(disp.float()))
    return out[:, :C] if pad else out


class _Correlation(torch.autograd.Function):
    @staticmethod
    def forward(ctx, left, right, ph, pw, keep):
        _require_gpu(left, right)
        if left.dim() != 4 or left.shape != right.shape:
            raise ValueError("reference_fm / target_fm must be [B,C,H,W] of equal shape")
        left, right = _lib.contiguous(left), _lib.contiguous(right)
        B, C, H, W = left.shape
        out = torch.empty((B, keep, H, W), device=left.device, dtype=torch.float32)
        _lib.check(_lib.lib().ts_correlation_fwd(_lib.ptr(left), _lib.ptr(right), _lib.ptr(out), B, C, H, W, ph, pw, keep, _stream()),
                   "ts_correlation_fwd")
        ctx.save_for_backward(left, right, out)
        ctx.meta = (ph, pw, keep)
        return out

    @staticmethod
    def backward(ctx, g):
        left, right, out = ctx.saved_tensors
        ph, pw, keep = ctx.meta
        B, C, H, W = left.shape
        gl = torch.empty_like(left) if ctx.needs_input_grad[0] else None
        gr = torch.empty_like(right) if ctx.needs_input_grad[1] else None
        g = _lib.contiguous(g)
        _lib.check(_lib.lib().ts_correlation_bwd(_lib.ptr(left), _lib.ptr(right), _lib.ptr(out), _lib.ptr(g),
                                                 _lib.ptr(gl), _lib.ptr(gr), B, C, H, W, ph, pw, keep, _stream()), "ts_correlation_bwd")
        return gl, gr, None, None, None


def _corr_args(kernel_size, stride, padding, dilation, dilation_patch):
    if (kernel_size, stride, padding, dilation, dilation_patch) != (1, 1, 0, 1, 1):
        raise NotImplementedError("native correlation: kernel_size=1, stride=1, padding=0, dilation=1, dilation_patch=1 "
                                  "(what the reference's callers pass)")


def correlation(reference_fm, target_fm, patch_size=1, kernel_size=1, stride=1, padding=0, dilation=1, dilation_patch=1):
    """aggregation/utils/correlation.py:10-29 (same arguments): [B, patch_size^2, H, W], plane ph*p+pw = correlation with the
    right pixel at (y + ph - p//2, x + pw - p//2), leaky_relu(0.1) applied.  Native replacement of the third-party sampler."""
    _corr_args(kernel_size, stride, padding, dilation, dilation_patch)
    if patch_size < 1 or patch_size % 2 != 1:
        raise ValueError("patch_size must be odd")
    return _Correlation.apply(reference_fm, target_fm, patch_size, patch_size, patch_size * patch_size)


def correlation1d(reference_fm, target_fm, max_disp=1, kernel_size=1, stride=1, padding=0, dilation=1, dilation_patch=1):
    """aggregation/utils/correlation.py:32-57 (same arguments): [B, max_disp, H, W]; plane k correlates the left pixel x with
    the right pixel x + k - (max_disp - 1), i.e. disparity max_disp - 1 - k."""
    _corr_args(kernel_size, stride, padding, dilation, dilation_patch)
    if max_disp < 1:
        raise ValueError("max_disp must be >= 1")
    return _Correlation.apply(reference_fm, target_fm, 1, 2 * max_disp - 1, max_disp)


# --------------------------------------------------------------------------------------- K3 convolutions
def _pad_last(t, n):
    if t.shape[-1] == n:
        return t.contiguous()
    out = t.new_zeros(t.shape[:-1] + (n,))
    out[..., :t.shape[-1]] = t
    return out


_CPAD = {}


def _cpad(n):
    if n not in _CPAD:
        _CPAD[n] = int(_lib.lib().ts_conv_cout_pad(n))
    return _CPAD[n]


class WeightLayouts:
    """Kernel layouts of the convolution weights of one training step, refreshed in ONE launch.

    Every convolution call needs its weight as [A][taps][pad(B)] (forward and backward-data each their own): issued one by one that
    is ~280 launches of `ts_conv_weight_layout` per T=2 step.  Inside `with layouts:` the first request for a (weight, order) pair
    runs that launch and registers the pair; `refresh()` -- called by the step after the optimizer has changed the weights -- then
    re-lays every registered pair with one `ts_conv_weight_layout_many` launch and later requests are dictionary look-ups.
    Keys are (data_ptr, shape, order): in-place updates (the optimizers') keep them valid; a weight that is REPLACED gets a new
    entry (the stale one is re-laid for nothing until `clear()`)."""

    def __init__(self, lazy=False):
        """lazy: `refresh()` launches nothing; a layout is redone by its first request after it (one small launch, as without the
        object) and shared by the later requests of the step -- for a replayed graph, where the one-launch refresh leaves the
        layouts cold in the cache by the time the convolutions read them (train.py)."""
        self.entries = {}           # key -> [weight, out, descriptor tuple, epoch]
        self.custom = {}            # key -> [weight, out, make, epoch]
        self._table = None
        self._dirty = False
        self._blocks = 1
        self.lazy = bool(lazy)
        self.epoch = 0

    def __enter__(self):
        global _LAYOUTS
        self._outer, _LAYOUTS = _LAYOUTS, self
        return self

    def __exit__(self, *exc):
        global _LAYOUTS
        _LAYOUTS = self._outer
        return False

    def clear(self):
        self.entries, self.custom, self._table, self._dirty = {}, {}, None, False

    def get(self, weight, a_dim, b_dim, flip):
        key = (weight.data_ptr(), tuple(weight.shape), a_dim, b_dim, bool(flip))
        e = self.entries.get(key)
        if e is None:
            if len(self.entries) >= 4096:       # someone feeds temporaries (each kept alive below): start over rather than grow
                self.clear()
            out, desc = _layout_now(weight, a_dim, b_dim, flip)
            self.entries[key] = e = [weight, out, desc, self.epoch]
            self._dirty = True
        elif self.lazy and e[3] != self.epoch:
            A, T, nb, bpad, sa, sb, st, fl = e[2]
            _lib.check(_lib.lib().ts_conv_weight_layout(_lib.ptr(e[0]), _lib.ptr(e[1]), A, T, nb, bpad, sa, sb, st, fl, _stream()),
                       "ts_conv_weight_layout")
            e[3] = self.epoch
        return e[1]

    def get_custom(self, weight, tag, make):
        """A kernel form of `weight` that is not a plain [A][taps][pad(B)] re-layout (the 3x3 form of a 4x4 transposed
        convolution): `make(weight, out=None) -> out` fills it; kept and refreshed (one launch each) like the table entries."""
        key = (weight.data_ptr(), tuple(weight.shape), tag)
        e = self.custom.get(key)
        if e is None:
            e = self.custom[key] = [weight, make(weight, None), make, self.epoch]
        elif self.lazy and e[3] != self.epoch:
            make(e[0], e[1])
            e[3] = self.epoch
        return e[1]

    def refresh(self):
        """Re-lay every registered weight from its current values (one launch on the current stream; lazy: on next use)."""
        self.epoch += 1
        if not self.lazy:
            for e in self.custom.values():
                e[2](e[0], e[1])
        if self.lazy or not self.entries:
            return
        if self._dirty:
            import numpy as np
            rec = np.zeros(len(self.entries), dtype=np.dtype([("w", "<u8"), ("out", "<u8"), ("A", "<i4"), ("T", "<i4"), ("nb", "<i4"),
                                                               ("bpad", "<i4"), ("sa", "<i8"), ("sb", "<i8"), ("st", "<i8"),
                                                               ("flip", "<i4"), ("reserved", "<i4")]))
            most = 1
            for i, (weight, out, d, _) in enumerate(self.entries.values()):
                rec[i] = (weight.data_ptr(), out.data_ptr()) + d + (0,)
                most = max(most, out.numel())
            dev = next(iter(self.entries.values()))[1].device
            self._table = torch.from_numpy(rec.view(np.uint8).reshape(-1)).to(dev)
            self._blocks = min(64, (most + 255) // 256)
            self._dirty = False
        _lib.check(_lib.lib().ts_conv_weight_layout_many(_lib.ptr(self._table), len(self.entries), self._blocks, _stream()),
                   "ts_conv_weight_layout_many")


_LAYOUTS = None


def _layout_now(weight, a_dim, b_dim, flip):
    weight = weight.detach()
    if not weight.is_contiguous():
        weight = weight.contiguous()
    d1 = weight.shape[1]
    T = weight[0, 0].numel()
    strides = (d1 * T, T)
    A, nb = weight.shape[a_dim], weight.shape[b_dim]
    bpad = _cpad(nb)
    out = torch.empty((A, T, bpad), device=weight.device, dtype=torch.float32)
    desc = (A, T, nb, bpad, strides[a_dim], strides[b_dim], 1, int(flip))
    _lib.check(_lib.lib().ts_conv_weight_layout(_lib.ptr(weight), _lib.ptr(out), A, T, nb, bpad, strides[a_dim], strides[b_dim], 1,
                                                int(flip), _stream()), "ts_conv_weight_layout")
    return out, desc


def _layout(weight, a_dim, b_dim, flip=False):
    """[A][taps][pad(B)] kernel layout of a conv weight [d0, d1, taps...] (ts_conv_weight_layout): A / B are which of the first two
    dimensions goes outermost / innermost.  Inside a `WeightLayouts` context the layouts are kept and refreshed together."""
    # only LEAVES (parameters) are registered: a temporary made per step -- the two halves of first_layer_split's weight -- would add a
    # fresh entry every step, each pinning its tensor, its layout and a table rebuild (+ pageable upload) until the 4096-entry clear
    if _LAYOUTS is not None and weight.is_contiguous() and weight.is_leaf:
        return _LAYOUTS.get(weight, a_dim, b_dim, flip)
    return _layout_now(weight, a_dim, b_dim, flip)[0]


def _shift_vec(bias, n):
    """[coutp] epilogue shift holding the bias (the kernels add it to the raw sum: scale stays 1)."""
    if bias is None:
        return None
    if bias.numel() == n and bias.is_contiguous():
        return bias.detach()                    # Cout is its own bucket (8, 16, 32, 64): nothing to pad, no launch
    v = torch.zeros(n, device=bias.device, dtype=torch.float32)
    v[:bias.numel()] = bias.detach()
    return v


# Train-mode (1,3,3) stride-1 layers on the bf16-split matrix form (csrc/conv3d.hip ig_conv_x6_kernel; fp32 products from six bf16
# products, error below the f32-input MFMA chain's: tests/test_conv_x6_gpu.py), forward and input gradient, where the inference
# engine would choose it too: >= 16 input channels, more than 8 output channels, a grid that fills the chip.  The split copy of the
# weights is made per call from the kernel layout (the parameters move every step).  TS_TRAIN_X6=0 for the A/B.
_TRAIN_X6 = __import__("os").environ.get("TS_TRAIN_X6", "1") != "0"
_TRAIN_X6_MIN_GRID = int(__import__("os").environ.get("TS_TRAIN_X6_MIN_GRID", "256"))


def _x6_conv(x, weight, wspec, y, B, Cin, Cout, D, H, W, dilation, shift=None, scale=None, act=0, addend=None):
    """y = act(scale * conv(x) + shift) through ts_conv3d_hw_x6_fwd when the shape qualifies; False when it does not.
    `weight`: the framework's (contiguous) parameter; wspec = (stride_ci, stride_co, stride_tap, flip) of the convolution being run
    inside it -- layout and bf16 split are ONE launch (ts_conv3d_hw_x6_weight_split_from)."""
    if not _TRAIN_X6 or Cin < 32 or not weight.is_contiguous():
        return False
    L = _lib.lib()
    if not L.ts_conv3d_hw_x6_supported(Cin, Cout, W, 1, dilation, 0):
        return False
    grid = ((H + 7) // 8) * ((W + 31) // 32) * D * B * ((Cout + 31) // 32)
    wsb = _q("ts_conv3d_hw_x6_workspace_bytes", B, Cin, Cout, D, H, W)
    if grid < _TRAIN_X6_MIN_GRID and not wsb:
        return False
    w6 = torch.empty(_q("ts_conv3d_hw_x6_weight_bytes", Cin, Cout), device=x.device, dtype=torch.uint8)
    _lib.check(L.ts_conv3d_hw_x6_weight_split_from(_lib.ptr(weight.detach()), _lib.ptr(w6), Cin, Cout, wspec[0], wspec[1], wspec[2], wspec[3],
                                                   _stream()), "ts_conv3d_hw_x6_weight_split_from")
    ws = torch.empty(wsb, device=x.device, dtype=torch.uint8) if wsb else None
    Ho, Wo = H, W
    rc = L.ts_conv3d_hw_x6_fwd(_lib.ptr(x), _lib.ptr(w6), _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(y), B, Cin, Cout, D, H, W, dilation,
                               int(act), 0.0, x.stride(0), x.stride(1), y.stride(0), y.stride(1), _lib.ptr(addend),
                               (Cout * Ho * Wo) if addend is not None else 0, _lib.ptr(ws), wsb, _stream())
    _lib.check(rc, "ts_conv3d_hw_x6_fwd")
    return True


def _hw_forward(x, weight, geom, bias=None, fold=None, act=0, addend=None):
    """Raw Conv3d (1,3,3) [padding == dilation] / ConvTranspose3d (1,3,3) stride 2, padding 1, output_padding 1 (+ bias); with
    `fold` = (scale, shift) the epilogue applies act(y * scale + shift) (an eval-mode BatchNorm folded in, bias included).
    geom = (stride, dilation, transposed).  Replaces F.conv3d / F.conv_transpose3d inside layers.Conv3d / ConvTranspose3d
    (reference: layers/basic_layers.py:194-235,340-388 reach cuDNN through the same two functionals)."""
    stride, dilation, transposed = geom
    _require_gpu(x, weight)
    x = x.contiguous()
    B, Cin, D, H, W = x.shape
    if transposed:                                   # weight [Cin, Cout, 1, 3, 3]
        Cout = weight.shape[1]
        Ho, Wo = 2 * H, 2 * W
    else:                                            # weight [Cout, Cin, 1, 3, 3]
        Cout = weight.shape[0]
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    y = torch.empty((B, Cout, D, Ho, Wo), device=x.device, dtype=torch.float32)
    sc, sh = fold if fold is not None else (None, _shift_vec(bias, _cpad(Cout)))
    if addend is not None:          # [B, Cout, 1, Ho, Wo] (or [B, Cout, Ho, Wo]): added to every depth plane's raw sum
        addend = _lib.contiguous(addend)
        if addend.numel() != B * Cout * Ho * Wo or transposed:
            raise ValueError("conv addend: one [B, Cout, Ho, Wo] plane per batch item (stride-1 / stride-2 forms only)")
    # (element (ci, co, tap) of [Cout, Cin, 1, 3, 3]: ci * 9 + co * Cin * 9 + tap)
    if stride == 1 and not transposed and _x6_conv(x, weight, (9, Cin * 9, 1, 0), y, B, Cin, Cout, D, H, W, dilation, sh, sc, act, addend):
        return x, y, (B, Cin, Cout, D, H, W, stride, dilation, transposed)
    w_t = _layout(weight, 0, 1) if transposed else _layout(weight, 1, 0)          # [ci][t][co]
    L = _lib.lib()
    wsb = _q("ts_conv3d_hw_workspace_bytes", B, Cin, Cout, D, H, W, stride, int(transposed))
    ws = torch.empty(wsb, device=x.device, dtype=torch.uint8) if wsb else None
    rc = L.ts_conv3d_hw_fwd(_lib.ptr(x), _lib.ptr(w_t), _lib.ptr(sc), _lib.ptr(sh), _lib.ptr(y), B, Cin, Cout, D, H, W, stride, dilation,
                            int(transposed), int(act), 0.0, x.stride(0), x.stride(1), y.stride(0), y.stride(1),
                            _lib.ptr(addend), (Cout * Ho * Wo) if addend is not None else 0, _lib.ptr(ws), wsb, _stream())
    _lib.check(rc, "ts_conv3d_hw_fwd")
    return x, y, (B, Cin, Cout, D, H, W, stride, dilation, transposed)


def _channel_sum(dy):
    """dy [B, C, ...] -> [C]: sum over batch and pixels (a convolution's bias gradient) on ts_channel_sum_fwd."""
    dy = dy if dy.is_contiguous() else dy.contiguous()
    B, C = dy.shape[0], dy.shape[1]
    N = dy.numel() // (B * C)
    out = torch.empty(C, device=dy.device, dtype=torch.float32)
    ws = torch.empty(_q("ts_bn_workspace_bytes", B, C, N), device=dy.device, dtype=torch.uint8)
    _lib.check(_lib.lib().ts_channel_sum_fwd(_lib.ptr(dy), _lib.ptr(out), _lib.ptr(ws), B, C, N, C * N, N, _stream()), "ts_channel_sum_fwd")
    return out


class WgradDefer:
    """The ~95 wgrad_finish launches of a training step's backward as ONE (ts_conv_wgrad_finish_many, csrc/conv3d.hip).

    Inside `with defer:` the weight-gradient calls of convolutions whose weight was used ONCE in the step's forward pass leave
    their partial sums in their workspaces (kept alive here) and return a dw that is written only by `flush()` -- called by the step
    after backward(), before anything reads a gradient.  Weights used more than once (the UNet image encoder runs on both views) are
    accumulated by autograd as soon as the second gradient arrives, so they keep the immediate finish: uses are counted during the
    forward pass.  Not for steps whose gradient buckets go out during backward (dist.GradientBuckets reads .grad from hooks)."""

    def __init__(self):
        self.uses = {}              # weight.data_ptr() -> forward uses in this step
        self.keep = []              # partial-sum workspaces awaiting the flush
        self._host = [None, None]
        self._dev = None
        self._turn = 0
        self._copied = [None, None]
        self.cap = 512 * 48

    def __enter__(self):
        global _WGRAD_DEFER
        self._outer, _WGRAD_DEFER = _WGRAD_DEFER, self
        self.uses = {}
        self.discard()             # nothing of an earlier, aborted step may reach this step's finish launch
        return self

    def __exit__(self, *exc):
        global _WGRAD_DEFER
        _WGRAD_DEFER = self._outer
        # flush() has run in a completed step; after an exception between the first deferred call and the flush (an OOM-skip loop, an
        # interrupt) the descriptors still name workspaces and dw tensors that are about to be freed: drop them WITHOUT launching
        self.discard()
        return False

    def discard(self):
        """Drops every pending deferred finish (the library's descriptor list and the workspaces kept for it) without launching."""
        import ctypes
        L = _lib.lib()
        if int(L.ts_conv_wgrad_pending()) != 0:
            scratch = (ctypes.c_char * self.cap)()
            n, blocks = ctypes.c_int(0), ctypes.c_int(0)
            L.ts_conv_wgrad_take(ctypes.cast(scratch, ctypes.c_void_p), self.cap, ctypes.byref(n), ctypes.byref(blocks))
        self.keep = []

    def used(self, weight):
        k = weight.data_ptr()
        self.uses[k] = self.uses.get(k, 0) + 1

    def single_use(self, weight):
        # a deferred dw is handed to autograd UNWRITTEN and filled by flush(): only sound when AccumulateGrad takes the tensor itself
        # (no gradient accumulated yet, no hook that would read or clone it first)
        # (a non-leaf -- a slice made inside the step -- hands its gradient to another backward node, which reads it at once)
        return (self.uses.get(weight.data_ptr(), 0) == 1 and weight.is_leaf and weight.grad is None
                and not getattr(weight, "_backward_hooks", None) and not getattr(weight, "_post_accumulate_grad_hooks", None))

    def flush(self):
        import ctypes
        L = _lib.lib()
        if int(L.ts_conv_wgrad_pending()) == 0:
            self.keep = []
            return
        dev = self.keep[0].device
        if self._dev is None:
            self._dev = torch.empty(self.cap, dtype=torch.uint8, device=dev)
            self._host = [torch.empty(self.cap, dtype=torch.uint8).pin_memory() for _ in range(2)]
        capturing = torch.cuda.is_current_stream_capturing()
        turn = self._turn
        if self._copied[turn] is not None and not capturing:
            self._copied[turn].synchronize()             # the upload that last read this pinned table has completed
        host = self._host[turn]
        n, blocks = ctypes.c_int(0), ctypes.c_int(0)
        _lib.check(L.ts_conv_wgrad_take(ctypes.c_void_p(host.data_ptr()), self.cap, ctypes.byref(n), ctypes.byref(blocks)), "ts_conv_wgrad_take")
        self._dev.copy_(host, non_blocking=True)
        if not capturing:
            ev = torch.cuda.Event()
            ev.record()
            self._copied[turn] = ev
            self._turn ^= 1
        _lib.check(L.ts_conv_wgrad_finish_many(_lib.ptr(self._dev), n.value, blocks.value, _stream()), "ts_conv_wgrad_finish_many")
        self.keep = []


_WGRAD_DEFER = None


def _wgrad_workspace(cin, cout, taps, device):
    """Partial-sum buffer of ``ts_conv3d_*_bwd_weight`` (symmetric in the channel counts' roles: the larger of
    the two orders covers the transposed form, which exchanges them)."""
    L = _lib.lib()
    n = max(_q("ts_conv3d_bwd_weight_workspace_bytes", cin, cout, taps), _q("ts_conv3d_bwd_weight_workspace_bytes", cout, cin, taps))
    return torch.empty(n // 4, dtype=torch.float32, device=device), n


def _wgrad_launch(launch, weight, ws, *args):
    """rc of the weight-gradient call launch(*args) whose partial sums go to `ws`.  Inside a `WgradDefer` context a weight used once
    in the step leaves its finish to that context's flush(), which keeps `ws` alive until then."""
    defer = _WGRAD_DEFER if (_WGRAD_DEFER is not None and _WGRAD_DEFER.single_use(weight)) else None
    if defer is None:
        return launch(*args)
    L = _lib.lib()
    was = L.ts_conv_wgrad_defer(1)                   # (this thread: backward runs on autograd's own)
    try:
        return launch(*args)
    finally:
        L.ts_conv_wgrad_defer(was)
        defer.keep.append(ws)


def _bwd_data_layout(weight, stride, transposed):
    """[co][t][ci] layout that ts_conv3d_{hw,d}_bwd_data reads."""
    if transposed:
        return _layout(weight, 1, 0)                 # = W_T[ci][co][t]
    if stride == 2:
        return _layout(weight, 0, 1)                 # taps as they are
    return _layout(weight, 0, 1, flip=True)          # stride 1: the same convolution of dy with the taps flipped


def _count_use(weight):
    """Counts a forward use of `weight` for the active `WgradDefer`, where a backward will follow (no_grad frames do not count)."""
    if _WGRAD_DEFER is not None and weight.requires_grad and torch.is_grad_enabled():
        _WGRAD_DEFER.used(weight)


def _hw_backward(x, weight, dy, geom, need_x, need_w):
    B, Cin, Cout, D, H, W, stride, dilation, transposed = geom
    dy = dy.contiguous()
    L = _lib.lib()
    dx = dw = None
    if need_x:
        dx = torch.empty_like(x)
        # stride 1: the input gradient is the same convolution of dy with the flipped taps, Cout -> Cin channels
        # (element (ci' = co, co' = ci, tap) of [Cout, Cin, 1, 3, 3]: ci' * Cin * 9 + co' * 9 + (8 - tap))
        if not (stride == 1 and not transposed and _x6_conv(dy, weight, (Cin * 9, 9, 1, 1), dx, B, Cout, Cin, D, H, W, dilation)):
            w_b = _bwd_data_layout(weight, stride, transposed)
            rc = L.ts_conv3d_hw_bwd_data(_lib.ptr(dy), _lib.ptr(w_b), _lib.ptr(dx), B, Cin, Cout, D, H, W, stride, dilation,
                                         int(transposed), dy.stride(0), dy.stride(1), dx.stride(0), dx.stride(1), _stream())
            _lib.check(rc, "ts_conv3d_hw_bwd_data")
    if need_w:
        dw = torch.empty_like(weight)
        ws, nws = _wgrad_workspace(Cin, Cout, 9, x.device)
        if transposed:         # roles exchanged: a stride-2 convolution maps dy (2H x 2W) to x
            rc = _wgrad_launch(L.ts_conv3d_hw_bwd_weight, weight, ws, _lib.ptr(dy), _lib.ptr(x), _lib.ptr(dw), B, Cout, Cin, D, 2 * H, 2 * W,
                               2, 1, dy.stride(0), dy.stride(1), x.stride(0), x.stride(1), _lib.ptr(ws), nws, _stream())
        else:
            rc = _wgrad_launch(L.ts_conv3d_hw_bwd_weight, weight, ws, _lib.ptr(x), _lib.ptr(dy), _lib.ptr(dw), B, Cin, Cout, D, H, W,
                               stride, dilation, x.stride(0), x.stride(1), dy.stride(0), dy.stride(1), _lib.ptr(ws), nws, _stream())
        _lib.check(rc, "ts_conv3d_hw_bwd_weight")
    return dx, dw


def _d_forward(x, weight, geom, bias=None, fold=None, act=0, addend=None):
    """Raw Conv3d (k,1,1) / ConvTranspose3d (3,1,1) stride 2, padding 1, output_padding 1 along D (+ bias in the kernel's epilogue);
    `fold`: see _hw_forward.  geom = (stride, dilation, padding, transposed)."""
    stride, dilation, padding, transposed = geom
    _require_gpu(x, weight)
    x = x.contiguous()
    B, Cin, Din, H, W = x.shape
    k = weight.shape[2]
    if transposed:
        Cout = weight.shape[1]
        w_t = _layout(weight, 0, 1)
        Dout = 2 * Din
    else:
        Cout = weight.shape[0]
        w_t = _layout(weight, 1, 0)
        Dout = (Din + 2 * padding - dilation * (k - 1) - 1) // stride + 1
    y = torch.empty((B, Cout, Dout, H, W), device=x.device, dtype=torch.float32)
    sc, sh = fold if fold is not None else (None, _shift_vec(bias, _cpad(Cout)))
    rc = _lib.lib().ts_conv3d_d_fwd(_lib.ptr(x), _lib.ptr(w_t), _lib.ptr(sc), _lib.ptr(sh), _lib.ptr(y), B, Cin, Cout, Din, H, W, k, stride,
                                    dilation, padding, int(transposed), int(act), 0.0, x.stride(0), x.stride(1), y.stride(0),
                                    y.stride(1), _stream())
    _lib.check(rc, "ts_conv3d_d_fwd")
    return x, y, (B, Cin, Cout, Din, H, W, k, stride, dilation, padding, transposed)


def _d_backward(x, weight, dy, geom, need_x, need_w):
    B, Cin, Cout, Din, H, W, k, stride, dilation, padding, transposed = geom
    dy = dy.contiguous()
    L = _lib.lib()
    dx = dw = None
    if need_x:
        w_b = _bwd_data_layout(weight, stride, transposed)
        dx = torch.empty_like(x)
        rc = L.ts_conv3d_d_bwd_data(_lib.ptr(dy), _lib.ptr(w_b), _lib.ptr(dx), B, Cin, Cout, Din, H, W, k, stride, dilation,
                                    padding, int(transposed), dy.stride(0), dy.stride(1), dx.stride(0), dx.stride(1), _stream())
        _lib.check(rc, "ts_conv3d_d_bwd_data")
    if need_w:
        dw = torch.empty_like(weight)
        ws, nws = _wgrad_workspace(Cin, Cout, k, x.device)
        if transposed:
            rc = _wgrad_launch(L.ts_conv3d_d_bwd_weight, weight, ws, _lib.ptr(dy), _lib.ptr(x), _lib.ptr(dw), B, Cout, Cin, 2 * Din, H, W,
                               3, 2, 1, 1, dy.stride(0), dy.stride(1), x.stride(0), x.stride(1), _lib.ptr(ws), nws, _stream())
        else:
            rc = _wgrad_launch(L.ts_conv3d_d_bwd_weight, weight, ws, _lib.ptr(x), _lib.ptr(dy), _lib.ptr(dw), B, Cin, Cout, Din, H, W, k,
                               stride, dilation, padding, x.stride(0), x.stride(1), dy.stride(0), dy.stride(1), _lib.ptr(ws), nws, _stream())
        _lib.check(rc, "ts_conv3d_d_bwd_weight")
    return dx, dw


_ONES = {}


def _ones(n, device):
    key = (n, device)
    if key not in _ONES:
        _ONES[key] = torch.ones(n, device=device, dtype=torch.float32)
    return _ONES[key]


def _zeros_const(n, device, _cache={}):
    key = (n, device)
    if key not in _cache:
        _cache[key] = torch.zeros(n, device=device, dtype=torch.float32)
    return _cache[key]


def _dc_conv3_weight(weight, out=None):
    """[Cin][Cout][4][4] -> [(4*Cout)][9][pad(Cin)]: weight of the 3x3 convolution that is d/dx of the transposed convolution."""
    Cin, Cout = weight.shape[0], weight.shape[1]
    cpad = _cpad(Cin)
    if out is None:
        out = torch.empty((4 * Cout, 9, cpad), device=weight.device, dtype=torch.float32)
    w = weight.detach()
    w = w if w.is_contiguous() else w.contiguous()
    _lib.check(_lib.lib().ts_deconv2d_k4s2_weight_to_conv3(_lib.ptr(w), _lib.ptr(out), Cin, Cout, cpad, _stream()),
               "ts_deconv2d_k4s2_weight_to_conv3")
    return out


def _dc_forward(x, weight, geom=None, bias=None, fold=None, act=0, addend=None):
    """Raw ConvTranspose2d(kernel 4, stride 2, padding 1) (+ bias) of UNet.deconv4 / deconv2 (module.py:453-457): ts_deconv2d_k4s2_fwd;
    `fold`: see _hw_forward.  The family has one geometry: geom is None."""
    _require_gpu(x, weight)
    x = x.contiguous()
    B, Cin, H, W = x.shape
    Cout = weight.shape[1]
    w_t = _layout(weight, 0, 1)                                                   # [ci][16 taps][pad(co)]
    pad = _cpad(Cout)
    y = torch.empty((B, Cout, 2 * H, 2 * W), device=x.device, dtype=torch.float32)
    if fold is not None:
        sc, sh = fold
    else:
        sc, sh = _ones(pad, x.device), (_shift_vec(bias, pad) if bias is not None else _zeros_const(pad, x.device))
    rc = _lib.lib().ts_deconv2d_k4s2_fwd(_lib.ptr(x), _lib.ptr(w_t), _lib.ptr(sc), _lib.ptr(sh), _lib.ptr(y),
                                         B, Cin, Cout, H, W, int(act), y.stride(0), _stream())
    _lib.check(rc, "ts_deconv2d_k4s2_fwd")
    return x, y, (B, Cin, Cout, H, W)


def _dc_backward(x, weight, dy, geom, need_x, need_w):
    """d/dx = conv3x3(space_to_depth2(dy)) with the weight's 3x3 form (four parity classes, two taps per axis each: 16 of the 36
    taps are non-zero), d/dW = the weight gradient of that same convolution gathered back to [Cin][Cout][4][4]: both on the MFMA
    convolution kernels of the (1,3,3) family (a plane = depth 1)."""
    B, Cin, Cout, H, W = geom
    dy = dy.contiguous()
    L = _lib.lib()
    z = torch.empty((B, 4 * Cout, H, W), device=dy.device, dtype=torch.float32)
    _lib.check(L.ts_space_to_depth2_fwd(_lib.ptr(dy), _lib.ptr(z), B, Cout, H, W, _stream()), "ts_space_to_depth2_fwd")
    dx = dw = None
    zc = 4 * Cout
    if need_x:
        if _LAYOUTS is not None and weight.is_contiguous():
            w3 = _LAYOUTS.get_custom(weight, "dc3", _dc_conv3_weight)
        else:
            w3 = _dc_conv3_weight(weight)
        dx = torch.empty_like(x)
        wsb = _q("ts_conv3d_hw_workspace_bytes", B, zc, Cin, 1, H, W, 1, 0)
        ws = torch.empty(wsb, device=x.device, dtype=torch.uint8) if wsb else None
        rc = L.ts_conv3d_hw_fwd(_lib.ptr(z), _lib.ptr(w3), None, None, _lib.ptr(dx), B, zc, Cin, 1, H, W, 1, 1, 0, 0, 0.0,
                                z.stride(0), z.stride(1), dx.stride(0), dx.stride(1), None, 0, _lib.ptr(ws), wsb, _stream())
        _lib.check(rc, "ts_conv3d_hw_fwd")
    if need_w:
        dw3 = torch.empty((Cin, zc, 9), device=x.device, dtype=torch.float32)
        ws, nws = _wgrad_workspace(zc, Cin, 9, x.device)
        rc = L.ts_conv3d_hw_bwd_weight(_lib.ptr(z), _lib.ptr(x), _lib.ptr(dw3), B, zc, Cin, 1, H, W, 1, 1,
                                       z.stride(0), z.stride(1), x.stride(0), x.stride(1), _lib.ptr(ws), nws, _stream())
        _lib.check(rc, "ts_conv3d_hw_bwd_weight")
        dw = torch.empty_like(weight)
        _lib.check(L.ts_deconv2d_k4s2_wgrad_from_conv3(_lib.ptr(dw3), _lib.ptr(dw), Cin, Cout, _stream()), "ts_deconv2d_k4s2_wgrad_from_conv3")
    return dx, dw


def deconv2d_k4s2_supported(weight_shape, stride, padding, output_padding, dilation, groups):
    """True when a ConvTranspose2d runs on the HIP kernels: kernel 4, stride 2, padding 1, <= 32 output and <= 64 input channels."""
    return (len(weight_shape) == 4 and tuple(weight_shape[2:]) == (4, 4) and tuple(stride) == (2, 2) and tuple(padding) == (1, 1) and
            tuple(output_padding) == (0, 0) and tuple(dilation) == (1, 1) and groups == 1 and weight_shape[1] <= 32 and weight_shape[0] <= 64)


class BNFolds:
    """Eval-mode BatchNorm of a training step folded into the convolution epilogue.  The frames a training step runs in eval() /
    no_grad (every previous frame, projects/TemporalStereo/TemporalStereo.py:268-274) need no batch statistics and no backward: their
    conv -> BatchNorm -> activation is ONE convolution launch with a per-channel scale / shift, as in the inference engine -- but the
    running statistics and the affine parameters move every step, so the folds are recomputed per step: `refresh()` does that for every
    registered layer in one launch (ts_bn_fold_many).  Inside `with folds:` an eval-mode, gradient-free wrapper call takes the fused
    form; its first call registers the layer (and folds it on the spot)."""

    def __init__(self):
        self.entries = {}           # key -> [gamma, beta, mean, var, bias, scale, shift, C, pad]
        self._table, self._dirty, self._eps = None, False, None

    def __enter__(self):
        global _FOLDS
        self._outer, _FOLDS = _FOLDS, self
        return self

    def __exit__(self, *exc):
        global _FOLDS
        _FOLDS = self._outer
        return False

    def _upload(self, entries):
        import numpy as np
        rec = np.zeros(len(entries), dtype=np.dtype([("gamma", "<u8"), ("beta", "<u8"), ("mean", "<u8"), ("var", "<u8"), ("bias", "<u8"),
                                                      ("scale", "<u8"), ("shift", "<u8"), ("C", "<i4"), ("pad", "<i4")]))
        for i, e in enumerate(entries):
            rec[i] = tuple(t.data_ptr() if t is not None else 0 for t in e[:7]) + (e[7], e[8])
        return torch.from_numpy(rec.view(np.uint8).reshape(-1)).to(entries[0][5].device)

    def get(self, gamma, beta, mean, var, bias, eps, cout):
        key = (mean.data_ptr(), var.data_ptr(), gamma.data_ptr() if gamma is not None else 0, bias.data_ptr() if bias is not None else 0)
        e = self.entries.get(key)
        if e is None:
            if self._eps is not None and float(eps) != self._eps:
                return None                                     # one eps per table (every BatchNorm of the model has the default)
            self._eps = float(eps)
            pad = _cpad(cout)
            e = [gamma, beta, mean, var, bias, torch.empty(pad, device=mean.device), torch.empty(pad, device=mean.device), int(cout), pad]
            self.entries[key] = e
            self._dirty = True
            _lib.check(_lib.lib().ts_bn_fold_many(_lib.ptr(self._upload([e])), 1, self._eps, _stream()), "ts_bn_fold_many")
        return e[5], e[6]

    def refresh(self):
        if not self.entries:
            return
        if self._dirty:
            self._table = self._upload(list(self.entries.values()))
            self._dirty = False
        _lib.check(_lib.lib().ts_bn_fold_many(_lib.ptr(self._table), len(self.entries), self._eps, _stream()), "ts_bn_fold_many")


_FOLDS = None
BN_ACT = {None: 0, "SiLU": 1, "ReLU": 2}
_COUNTS = {}


def _count_const(n, device):
    key = (float(n), device)
    if key not in _COUNTS:
        _COUNTS[key] = torch.full((1,), float(n), device=device, dtype=torch.float32)
    return _COUNTS[key]


def _all_gather_flat(out, part, group):
    """out [world * n] <- every rank's part [n] (all_gather_into_tensor where the backend has it: RCCL; a list gather otherwise)."""
    import torch.distributed as dist
    try:
        dist.all_gather_into_tensor(out, part, group=group)
    except (RuntimeError, NotImplementedError):
        world = dist.get_world_size(group)
        parts = [out[i * part.numel():(i + 1) * part.numel()] for i in range(world)]
        tmp = [torch.empty_like(part) for _ in range(world)]
        dist.all_gather(tmp, part, group=group)
        for d, t in zip(parts, tmp):
            d.copy_(t)


import os as _os
_BN_FUSED = _os.environ.get("TS_BN_FUSED", "1") != "0"
_BN_FEW_VALUES = 4096       # csrc/spp3d.hip kSmallBnMax
_EXCHANGES = [0]            # SyncBatchNorm exchanges issued by this process (forward all_gathers + backward all_reduces; bench.py reports them per step)


def _peer_group(group, n_floats):
    """The installed peer-mailbox group (peer.install) when it spans `group` and carries `n_floats` per exchange, else None:
    torch.distributed collectives (a SyncBatchNorm over a sub-group, or with C >= 512, never goes through the wrong mailboxes)."""
    from . import peer
    return peer.for_group(group, n_floats)


def _bn_act_forward(y, gamma, beta, running_mean, running_var, eps, momentum, act, training, group, counter):
    """(out, mean, var, n_total): out = act(BatchNorm(y)) over a raw convolution output y [B, C, ...], the BatchNorm tail of _ConvBNAct and
    _DecoderConv.  Train mode: batch statistics, the running ones and `counter` updated by the statistics launch; over a `group` of
    several ranks the statistics are exchanged (one all_gather) and n_total is 1 / (global count) as a device scalar.  Eval mode:
    mean / var are the running statistics.  (mean, var, n_total) are what _bn_act_backward needs."""
    B, C = y.shape[0], y.shape[1]
    N = y.numel() // (B * C)
    L = _lib.lib()
    n_total = float(B * N)
    out = torch.empty_like(y)
    if training and group is None and _BN_FUSED:
        # single rank: statistics and their use in two launches (ts_bn_train_fwd)
        mean = torch.empty(C, device=y.device, dtype=torch.float32)
        var = torch.empty_like(mean)
        ws = torch.empty(_q("ts_bn_workspace_bytes", B, C, N), device=y.device, dtype=torch.uint8)
        _lib.check(L.ts_bn_train_fwd(_lib.ptr(y), _lib.ptr(mean), _lib.ptr(var), _lib.ptr(running_mean), _lib.ptr(running_var),
                                     float(momentum), _lib.ptr(counter), _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(out), _lib.ptr(ws),
                                     B, C, N, y.stride(0), y.stride(1), out.stride(0), out.stride(1), float(eps), int(act), _stream()),
                   "ts_bn_train_fwd")
        return out, mean, var, n_total
    if training:
        if group is not None:       # the statistics kernel writes straight into the record that is exchanged: [mean | var | count]
            pack = torch.empty(2 * C + 1, device=y.device, dtype=torch.float32)
            mean, var = pack[:C], pack[C:2 * C]
        else:
            mean = torch.empty(C, device=y.device, dtype=torch.float32)
            var = torch.empty_like(mean)
        ws = torch.empty(_q("ts_bn_workspace_bytes", B, C, N), device=y.device, dtype=torch.uint8)
        local_update = group is None and running_mean is not None
        _lib.check(L.ts_bn_stats_fwd(_lib.ptr(y), _lib.ptr(mean), _lib.ptr(var), _lib.ptr(running_mean if local_update else None),
                                     _lib.ptr(running_var if local_update else None), float(momentum), _lib.ptr(counter),
                                     _lib.ptr(ws), B, C, N, y.stride(0), y.stride(1), _stream()), "ts_bn_stats_fwd")
        if group is not None:
            # one all_gather of [mean | var | count], merged on the device (ts_bn_sync_merge); the total count stays there too
            import torch.distributed as dist
            world = dist.get_world_size(group)
            pack[2 * C:].copy_(_count_const(n_total, y.device))
            allp = torch.empty(world * (2 * C + 1), device=y.device, dtype=torch.float32)
            pg = _peer_group(group, 2 * C + 1)
            if pg is not None:      # one kernel over the peer-mapped mailboxes (csrc/peer.hip): no communicator launch, capturable
                pg.all_gather(pack, allp)
            else:
                _all_gather_flat(allp, pack, group)
            _EXCHANGES[0] += 1
            mean, var = torch.empty_like(mean), torch.empty_like(var)
            inv_n = torch.empty(1, device=y.device, dtype=torch.float32)
            _lib.check(L.ts_bn_sync_merge(_lib.ptr(allp), world, C, _lib.ptr(mean), _lib.ptr(var), _lib.ptr(running_mean), _lib.ptr(running_var),
                                          float(momentum), _lib.ptr(inv_n), _stream()), "ts_bn_sync_merge")
            n_total = inv_n                       # a device scalar from here on (backward scales its sums with it)
    else:
        mean, var = running_mean, running_var
    _lib.check(L.ts_bn_apply_act_fwd(_lib.ptr(y), _lib.ptr(mean), _lib.ptr(var), _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(out),
                                     B, C, N, y.stride(0), y.stride(1), out.stride(0), out.stride(1), float(eps), int(act),
                                     _stream()), "ts_bn_apply_act_fwd")
    return out, mean, var, n_total


def _bn_act_backward(y, g, mean, var, gamma, beta, eps, act, training, group, n_total, few):
    """(dy, ggamma, gbeta) of _bn_act_forward for the output gradient g (contiguous); the pre-activation is recomputed from y.  ggamma /
    gbeta are THIS rank's sums (a gradient exchange averages them), None without affine parameters; over a `group` the two sums that dy
    needs are exchanged (one all_reduce).  few: ts_bn_small_train_bwd (fp64 inside), for a single rank and at most _BN_FEW_VALUES values
    per channel -- SPP3D's coarse levels have down to two, where the gradient is what a cancellation leaves."""
    B, C = y.shape[0], y.shape[1]
    N = y.numel() // (B * C)
    L = _lib.lib()
    s1 = torch.empty(C, device=y.device, dtype=torch.float32)
    s2 = torch.empty_like(s1)
    ggamma, gbeta = (s2, s1) if gamma is not None else (None, None)
    if few:
        dy = torch.empty_like(y)
        _lib.check(L.ts_bn_small_train_bwd(_lib.ptr(y), _lib.ptr(g), _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(s1), _lib.ptr(s2), _lib.ptr(dy),
                                           B, C, N, y.stride(0), y.stride(1), g.stride(0), g.stride(1), dy.stride(0), dy.stride(1),
                                           eps, act, _stream()), "ts_bn_small_train_bwd")
        return dy, ggamma, gbeta
    ws = torch.empty(_q("ts_bn_workspace_bytes", B, C, N), device=y.device, dtype=torch.uint8)
    if training and group is None and _BN_FUSED:
        dy = torch.empty_like(y)
        _lib.check(L.ts_bn_train_bwd(_lib.ptr(y), _lib.ptr(g), _lib.ptr(mean), _lib.ptr(var), _lib.ptr(gamma), _lib.ptr(beta),
                                     _lib.ptr(s1), _lib.ptr(s2), _lib.ptr(dy), _lib.ptr(ws), B, C, N, y.stride(0), y.stride(1),
                                     g.stride(0), g.stride(1), eps, act, n_total, _stream()), "ts_bn_train_bwd")
        return dy, ggamma, gbeta
    _lib.check(L.ts_bn_act_bwd_reduce(_lib.ptr(y), _lib.ptr(g), _lib.ptr(mean), _lib.ptr(var), _lib.ptr(gamma), _lib.ptr(beta),
                                      _lib.ptr(s1), _lib.ptr(s2), _lib.ptr(ws), B, C, N, y.stride(0), y.stride(1), g.stride(0),
                                      g.stride(1), eps, act, _stream()), "ts_bn_act_bwd_reduce")
    t1, t2 = s1, s2
    count = n_total
    if training and group is not None:
        import torch.distributed as dist
        pack = torch.cat([s1, s2])
        pg = _peer_group(group, 2 * C)
        if pg is not None:
            pg.all_reduce_sum(pack, scale=n_total)               # summed in rank order and scaled inside the exchange kernel
        else:
            dist.all_reduce(pack, op=dist.ReduceOp.SUM, group=group)
            pack = pack * n_total                                # n_total is 1 / (global count) on the device here: pre-scaled sums,
        t1, t2, count = pack[:C], pack[C:], 1.0                  # the kernel's own division is by 1 (no host read of a count)
        _EXCHANGES[0] += 1
    dy = torch.empty_like(y)
    _lib.check(L.ts_bn_act_bwd_apply(_lib.ptr(y), _lib.ptr(g), _lib.ptr(mean), _lib.ptr(var), _lib.ptr(gamma), _lib.ptr(beta),
                                     _lib.ptr(t1), _lib.ptr(t2), _lib.ptr(dy), B, C, N, y.stride(0), y.stride(1), g.stride(0),
                                     g.stride(1), eps, act, int(training), count, _stream()), "ts_bn_act_bwd_apply")
    return dy, ggamma, gbeta


class _ConvBNAct(torch.autograd.Function):
    """conv -> BatchNorm -> activation of the reference's wrappers (layers/basic_layers.py:194-235: conv, then `self.norm`, then
    `self.activation`) as ONE autograd node on HIP kernels: the convolution of the family's _FAMILIES entry (bias in its epilogue), then
    _bn_act_forward; backward _bn_act_backward (nothing but the raw convolution output is kept), then the family's data / weight
    gradients.  `group`: a torch.distributed process group -- statistics and the two backward sums are exchanged across its ranks
    (SyncBatchNorm of dist.py, one all_gather forward, one all_reduce backward)."""

    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, addend, spec):
        # backward returns one gradient per argument, in this order: (x, weight, bias, gamma, beta, addend, spec -> None).
        # spec: everything that takes no gradient, packed by conv_bn_act.
        # addend (families with the flag only): [B, Cout, 1, Ho, Wo], added to every depth plane of the raw convolution (first_layer_split)
        # few_values: see _bn_act_backward (train mode on a single rank only)
        family, geom, running_mean, running_var, counter, eps, momentum, act, training, group, may_fold, few_values = spec
        fam = _FAMILIES[family]
        if addend is not None and not fam.takes_addend:
            raise ValueError("conv_bn_act: an addend needs the (1,3,3) family")
        # may_fold is decided by conv_bn_act in the CALLER's grad mode (inside Function.forward grad mode is always off): the folded
        # path keeps nothing for backward, so it is for calls through which no gradient can flow
        if _FOLDS is not None and not training and may_fold and running_mean is not None:
            fold = _FOLDS.get(gamma, beta, running_mean, running_var, bias, eps, fam.cout(weight, geom))
            if fold is not None:        # eval frame of a training step: conv -> BatchNorm -> activation in the convolution's epilogue
                return fam.forward(x, weight, geom, None, fold, act, addend)[1]
        x, y, cg = fam.forward(x, weight, geom, bias, None, 0, addend)
        out, mean, var, n_total = _bn_act_forward(y, gamma, beta, running_mean, running_var, eps, momentum, act, training, group, counter)
        few = bool(few_values) and training and group is None and 2 <= y.numel() // y.shape[1] <= _BN_FEW_VALUES
        ctx.save_for_backward(x, weight, y, mean, var, gamma, beta)
        ctx.meta = (fam, cg, float(eps), int(act), bool(training), group, n_total, few, bias is not None, addend is not None)
        return out

    @staticmethod
    def backward(ctx, g):
        x, weight, y, mean, var, gamma, beta = ctx.saved_tensors
        fam, cg, eps, act, training, group, n_total, few, has_bias, has_addend = ctx.meta
        need_x, need_w, need_bias, _, _, need_addend, _ = ctx.needs_input_grad
        dy, ggamma, gbeta = _bn_act_backward(y, g.contiguous(), mean, var, gamma, beta, eps, act, training, group, n_total, few)
        dx, dw = fam.backward(x, weight, dy, cg, need_x, need_w)
        gbias = gadd = None
        if has_bias and need_bias:
            gbias = _channel_sum(dy)                               # == 0 up to rounding in train mode (BatchNorm removes the mean)
        if has_addend and need_addend:
            gadd = dy.sum(dim=2, keepdim=True)                     # the D-invariant term reaches every depth plane
        return dx, dw, gbias, ggamma, gbeta, gadd, None


def conv_bn_act(x, weight, bias, bn, activation, family, geom, transposed=False, addend=None, few_values=False):
    """Fused wrapper forward (see _ConvBNAct).  `bn`: an nn.BatchNorm*d / dist.SyncBatchNorm module; `activation`: None | 'SiLU' |
    'ReLU'; family 'hw' geom (stride, dilation, transposed) / family 'd' geom (stride, dilation, padding, transposed) / family 'hw3'
    (3x3x3, stride 1, padding 1: three (1,3,3) launches and a depth sum, see _hw3_forward) geom (1, 1, False) / family 'dc'
    (ConvTranspose2d kernel 4, stride 2, padding 1) geom None: the keys of _FAMILIES."""
    # parameters / buffers straight from the module's dictionaries: nn.Module.__getattr__ (the fallback every `bn.weight`,
    # `bn.running_mean` ... goes through) was ~10 lookups x 180 wrappers per frame
    _count_use(weight)
    d, P, Bf = bn.__dict__, bn._parameters, bn._buffers
    rmean = Bf.get("running_mean")
    training = d["training"] or rmean is None
    group = None
    if training and "process_group" in d:
        import torch.distributed as dist
        pg = d["process_group"]
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(pg) > 1:
            group = pg if pg is not None else dist.group.WORLD
    momentum = d["momentum"] if d["momentum"] is not None else 0.1
    counter = Bf.get("num_batches_tracked") if (training and d["track_running_stats"]) else None     # incremented by the statistics launch
    gamma, beta = P["weight"], P["bias"]
    may_fold = (not training) and (not torch.is_grad_enabled() or not any(
        t is not None and t.requires_grad for t in (x, weight, bias, gamma, beta, addend)))
    return _ConvBNAct.apply(x, weight, bias, gamma, beta, addend, (family, geom, rmean, Bf.get("running_var"), counter, d["eps"], momentum,
                                                                   BN_ACT[activation], training, group, may_fold, few_values))


def conv3d_supported(weight_shape, stride, padding, dilation, groups, transposed=False, output_padding=(0, 0, 0)):
    """'hw' | 'd' | None: which HIP family runs a Conv3d / ConvTranspose3d with these hyper-parameters."""
    if groups != 1 or len(weight_shape) != 5:
        return None
    kd, kh, kw = weight_shape[2:]
    cout = weight_shape[1] if transposed else weight_shape[0]
    cin = weight_shape[0] if transposed else weight_shape[1]
    if max(cout, cin if transposed else 0) > 64:
        return None                                     # the weight-gradient kernel holds <= 64 output channels
    if (kd, kh, kw) == (1, 3, 3) and stride[0] == 1 and stride[1] == stride[2] and dilation[1] == dilation[2] and \
            padding[0] == 0 and dilation[0] == 1:
        s, d = stride[1], dilation[1]
        if transposed:
            ok = s == 2 and d == 1 and tuple(padding[1:]) == (1, 1) and tuple(output_padding) == (0, 1, 1)
        else:
            ok = tuple(padding[1:]) == (d, d) and (s, d) in ((1, 1), (1, 2), (2, 1))
        return "hw" if ok else None
    if kh == 1 and kw == 1 and kd in (1, 3, 5) and tuple(stride[1:]) == (1, 1) and tuple(padding[1:]) == (0, 0):
        s, d, pd = stride[0], dilation[0], padding[0]
        if transposed:
            ok = kd == 3 and s == 2 and d == 1 and pd == 1 and tuple(output_padding) == (1, 0, 0)
        else:
            ok = s == 1 or (s == 2 and kd == 3 and d == 1 and pd == 1)
        return "d" if ok else None
    return None


def conv3d(x, weight, bias=None, stride=(1, 1, 1), padding=(0, 0, 0), dilation=(1, 1, 1)):
    """F.conv3d on the HIP kernels for the (1,3,3) / (k,1,1) families (fp32, GPU)."""
    kind = conv3d_supported(tuple(weight.shape), stride, padding, dilation, 1)
    _count_use(weight)
    if kind == "hw":
        y = _ConvRaw.apply(x, weight, None, "hw", (stride[1], dilation[1], False))
    elif kind == "d":
        return _ConvRaw.apply(x, weight, bias, "d", (stride[0], dilation[0], padding[0], False))       # bias in the epilogue
    else:
        raise NotImplementedError("conv3d: kernel %s stride %s padding %s dilation %s has no HIP kernel"
                                  % (tuple(weight.shape[2:]), stride, padding, dilation))
    return y if bias is None else y + bias.view(1, -1, 1, 1, 1)


def conv_transpose3d(x, weight, bias=None, stride=(1, 2, 2), padding=(0, 1, 1), output_padding=(0, 1, 1)):
    """F.conv_transpose3d on the HIP kernels: (1,3,3) stride (1,2,2) or (3,1,1) stride (2,1,1), padding 1, output_padding 1."""
    kind = conv3d_supported(tuple(weight.shape), stride, padding, (1, 1, 1), 1, True, output_padding)
    _count_use(weight)
    if kind == "hw":
        y = _ConvRaw.apply(x, weight, None, "hw", (2, 1, True))
    elif kind == "d":
        y = _ConvRaw.apply(x, weight, None, "d", (2, 1, 1, True))
    else:
        raise NotImplementedError("conv_transpose3d: kernel %s stride %s padding %s output_padding %s has no HIP kernel"
                                  % (tuple(weight.shape[2:]), stride, padding, output_padding))
    return y if bias is None else y + bias.view(1, -1, 1, 1, 1)


# ---------------------------------------------------------------------------------------------- SPP3D
# (The slice launches are spelt out in _hw3_slice_conv rather than routed through _hw_forward / _hw_backward: those take a whole
# (1,3,3) weight, allocate their own outputs and are shared by every layer of the model; the slice's weight layout goes through the
# same WeightLayouts table, so a training step lays each slice out once.)
# 3x3x3 convolution (stride 1, padding 1) as three (1,3,3) convolutions: y[d] = Z_0[d-1] + Z_1[d] + Z_2[d+1] with Z_kd the (1,3,3)
# convolution of x with weight[:, :, kd] (family "hw3" of conv_bn_act; SPP3D.fuse[0], utils/SPP3D.py:34).  The slice of the weight is
# never copied: element (ci, co, tap) of slice kd sits at kd * 9 + ci * 27 + co * Cin * 27 + tap of the parameter.
def _hw3_check(x, weight):
    _require_gpu(x, weight)
    if weight.dim() != 5 or tuple(weight.shape[2:]) != (3, 3, 3) or weight.shape[0] > 64 or x.dim() != 5 or x.shape[1] != weight.shape[1]:
        raise ValueError("conv3d_k333: weight [Cout <= 64, Cin, 3, 3, 3] and x [B, Cin, D, H, W] (got %s and %s)"
                         % (tuple(weight.shape), tuple(x.shape)))


def _hw3_slice_conv(src, weight, kd, dst, B, Cin, Cout, D, H, W, backward):
    """dst = (1,3,3) convolution of src with slice kd of the 3x3x3 `weight` [Cout, Cin, 3, 3, 3] (contiguous); backward: the data
    gradient of that convolution (src = dy with Cout channels, dst with Cin, taps flipped in the plane)."""
    L = _lib.lib()
    wv = weight.detach().reshape(-1)[kd * 9:]
    cin, cout = (Cout, Cin) if backward else (Cin, Cout)                # of the convolution that is launched
    wspec = (Cin * 27, 27, 1, 1) if backward else (27, Cin * 27, 1, 0)
    if _x6_conv(src, wv, wspec, dst, B, cin, cout, D, H, W, 1):
        return
    bpad = _cpad(cout)

    def make(w, out=None):          # [cin][9][pad(cout)] of the slice, from its strides inside the parameter
        if out is None:
            out = torch.empty((cin, 9, bpad), device=w.device, dtype=torch.float32)
        _lib.check(L.ts_conv_weight_layout(_lib.ptr(w.detach().reshape(-1)[kd * 9:]), _lib.ptr(out), cin, 9, cout, bpad, wspec[0], wspec[1], 1,
                                           wspec[3], _stream()), "ts_conv_weight_layout")
        return out
    # kept and refreshed with the other layouts of a training step (WeightLayouts.get_custom), parameters only -- as _layout does
    w_t = _LAYOUTS.get_custom(weight, "hw3/%d/%d" % (kd, int(backward)), make) if (_LAYOUTS is not None and weight.is_leaf) else make(weight)
    if backward:
        rc = L.ts_conv3d_hw_bwd_data(_lib.ptr(src), _lib.ptr(w_t), _lib.ptr(dst), B, Cin, Cout, D, H, W, 1, 1, 0, src.stride(0), src.stride(1),
                                     dst.stride(0), dst.stride(1), _stream())
        _lib.check(rc, "ts_conv3d_hw_bwd_data")
        return
    wsb = _q("ts_conv3d_hw_workspace_bytes", B, Cin, Cout, D, H, W, 1, 0)
    ws = torch.empty(wsb, device=src.device, dtype=torch.uint8) if wsb else None
    rc = L.ts_conv3d_hw_fwd(_lib.ptr(src), _lib.ptr(w_t), None, None, _lib.ptr(dst), B, Cin, Cout, D, H, W, 1, 1, 0, 0, 0.0,
                            src.stride(0), src.stride(1), dst.stride(0), dst.stride(1), None, 0, _lib.ptr(ws), wsb, _stream())
    _lib.check(rc, "ts_conv3d_hw_fwd")


def _depth_sum3(z0, z1, z2, y, scale=None, shift=None, act=0):
    B, C, D, H, W = y.shape
    rc = _lib.lib().ts_depth_sum3_fwd(_lib.ptr(z0), _lib.ptr(z1), _lib.ptr(z2), _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(y), B, C, D, H, W,
                                      int(act), z0.stride(0), z0.stride(1), z1.stride(0), z1.stride(1), z2.stride(0), z2.stride(1),
                                      y.stride(0), y.stride(1), _stream())
    _lib.check(rc, "ts_depth_sum3_fwd")


def _hw3_forward(x, weight, geom=None, bias=None, fold=None, act=0, addend=None):
    """Raw Conv3d 3x3x3, stride 1, padding 1 (+ bias): three (1,3,3) launches and ts_depth_sum3_fwd each way; `fold`: see _hw_forward
    (applied by the depth sum's epilogue).  The family has one geometry: geom is not read."""
    _hw3_check(x, weight)
    x = x.contiguous()
    weight = weight if weight.is_contiguous() else weight.contiguous()
    B, Cin, D, H, W = x.shape
    Cout = weight.shape[0]
    y = torch.empty((B, Cout, D, H, W), device=x.device, dtype=torch.float32)
    _hw3_slice_conv(x, weight, 1, y, B, Cin, Cout, D, H, W, False)         # the centre slice straight into y
    z0 = z2 = y                                                             # D == 1: neither neighbour is read
    if D > 1:
        z0, z2 = torch.empty_like(y), torch.empty_like(y)
        _hw3_slice_conv(x, weight, 0, z0, B, Cin, Cout, D, H, W, False)
        _hw3_slice_conv(x, weight, 2, z2, B, Cin, Cout, D, H, W, False)
    sc, sh = fold if fold is not None else (None, bias.detach().contiguous() if bias is not None else None)
    if D > 1 or sc is not None or sh is not None or act:
        _depth_sum3(z0, y, z2, y, sc, sh, act)
    return x, y, (B, Cin, Cout, D, H, W)


def _hw3_backward(x, weight, dy, geom, need_x, need_w):
    B, Cin, Cout, D, H, W = geom
    dy = dy.contiguous()
    weight = weight if weight.is_contiguous() else weight.contiguous()
    L = _lib.lib()
    dx = dw = None
    if need_x:          # y[d] takes x[d + kd - 1] through slice kd, so dx[e] = G_0[e+1] + G_1[e] + G_2[e-1]: the same sum, ends exchanged
        dx = torch.empty_like(x)
        _hw3_slice_conv(dy, weight, 1, dx, B, Cin, Cout, D, H, W, True)
        if D > 1:
            g0, g2 = torch.empty_like(dx), torch.empty_like(dx)
            _hw3_slice_conv(dy, weight, 0, g0, B, Cin, Cout, D, H, W, True)
            _hw3_slice_conv(dy, weight, 2, g2, B, Cin, Cout, D, H, W, True)
            _depth_sum3(g2, dx, g0, dx)
    if need_w:          # slice kd: the (1,3,3) weight gradient of planes x[kd-1 ...] against dy[...]: depth-offset views, D - 1 planes
        parts = torch.empty((3, Cout, Cin, 9), device=x.device, dtype=torch.float32)
        ws, nws = _wgrad_workspace(Cin, Cout, 9, x.device)
        plane = H * W * 4
        for kd in range(3):
            nd = D if kd == 1 else D - 1
            if nd == 0:
                parts[kd].zero_()
                continue
            xo, go = (plane if kd == 2 else 0), (plane if kd == 0 else 0)
            rc = L.ts_conv3d_hw_bwd_weight(_lib.ptr(x) + xo, _lib.ptr(dy) + go, _lib.ptr(parts[kd]), B, Cin, Cout, nd, H, W, 1, 1,
                                           x.stride(0), x.stride(1), dy.stride(0), dy.stride(1), _lib.ptr(ws), nws, _stream())
            _lib.check(rc, "ts_conv3d_hw_bwd_weight")
        dw = parts.view(3, Cout, Cin, 3, 3).permute(1, 2, 0, 3, 4).contiguous()
    return dx, dw


# ---------------------------------------------------------------------------------------------- convolution families
class _ConvFamily:
    """One convolution family of the raw node (_ConvRaw) and of the fused node (_ConvBNAct):
    forward(x, weight, geom, bias, fold, act, addend) -> (x as the kernels read it, y, saved_geom)
    backward(x, weight, dy, saved_geom, need_x, need_w) -> (dx, dw)
    cout(weight, geom): output channels, from the weight alone (what a BatchNorm fold is sized by before anything runs)
    takes_addend: whether forward accepts a per-item plane added to the raw sum (first_layer_split).
    `geom` is the caller's tuple, named by the family's forward; `saved_geom` is the forward's own record for its backward."""
    __slots__ = ("forward", "backward", "cout", "takes_addend")

    def __init__(self, forward, backward, cout, takes_addend=False):
        self.forward, self.backward, self.cout, self.takes_addend = forward, backward, cout, takes_addend


def _cout_dim0(weight, geom):
    return weight.shape[0]


def _cout_dim1(weight, geom):
    return weight.shape[1]


def _cout_by_geom(weight, geom):            # geom[-1]: transposed, weight [Cin, Cout, ...]
    return weight.shape[1] if geom[-1] else weight.shape[0]


_FAMILIES = {
    "hw": _ConvFamily(_hw_forward, _hw_backward, _cout_by_geom, takes_addend=True),     # (1,3,3); geom (stride, dilation, transposed)
    "d": _ConvFamily(_d_forward, _d_backward, _cout_by_geom),                           # (k,1,1); geom (stride, dilation, padding, transposed)
    "dc": _ConvFamily(_dc_forward, _dc_backward, _cout_dim1),                           # ConvTranspose2d kernel 4, stride 2; geom None
    "hw3": _ConvFamily(_hw3_forward, _hw3_backward, _cout_dim0),                        # 3x3x3 as three (1,3,3) slices; geom not read
}


class _ConvRaw(torch.autograd.Function):
    """A raw convolution of any family (no scale / shift / activation; `bias`, where given, in the family's epilogue) as one autograd
    node: the family's forward, its data / weight gradients, ts_channel_sum_fwd for the bias."""

    @staticmethod
    def forward(ctx, x, weight, bias, family, geom):
        ctx.family = fam = _FAMILIES[family]
        x, y, ctx.geom = fam.forward(x, weight, geom, bias, None, 0, None)
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        need_x, need_w, need_bias, _, _ = ctx.needs_input_grad
        dx, dw = ctx.family.backward(x, weight, dy, ctx.geom, need_x, need_w)
        gb = _channel_sum(dy) if (ctx.has_bias and need_bias) else None
        return dx, dw, gb, None, None


def conv_transpose2d_k4s2(x, weight, bias=None):
    """F.conv_transpose2d(x, weight, bias, stride 2, padding 1) for 4x4 kernels on the HIP kernels (forward and backward; UNet.deconv2,
    module.py:457)."""
    return _ConvRaw.apply(x, weight, bias, "dc", None)


def conv3d_k333(x, weight):
    """F.conv3d(x, weight, None, stride 1, padding 1) for a 3x3x3 kernel (groups 1, dilation 1, <= 64 output channels) on the (1,3,3)
    HIP kernels.  `layers.Conv3d` does not choose it by itself (conv3d_supported is unchanged): SPP3D does."""
    return _ConvRaw.apply(x, weight, None, "hw3", None)


# ---------------------------------------------------------------------------------------------- SPP3D: pooling and expansion
_SPP_MAX_LEVELS = 4            # csrc/spp3d.hip kMaxLevels


def _spp_strides(strides):
    s = tuple(int(v) for v in strides)
    if not 1 <= len(s) <= _SPP_MAX_LEVELS or min(s) < 1:
        raise ValueError("spp3d: 1..%d strides >= 1 (got %s)" % (_SPP_MAX_LEVELS, (s,)))
    return s


def spp3d_level_sizes(size, strides):
    """[(n_d, n_h, n_w)] of the pooled levels of a (D, H, W) volume: box min(dim, s), floor(dim / box) cells (utils/SPP3D.py:42-43)."""
    return [tuple(n // min(n, s) for n in size) for s in strides]


def _spp_dense(t):
    """The kernels take batch / channel strides; D*H*W itself is dense."""
    D, H, W = t.shape[2:]
    return t if tuple(t.stride()[2:]) == (H * W, W, 1) and t.stride(1) >= D * H * W and (t.shape[0] == 1 or t.stride(0) >= t.stride(1) * (t.shape[1] - 1) + D * H * W) \
        else t.contiguous()


class _Spp3dPool(torch.autograd.Function):
    """Every avg_pool3d of SPP3D.forward (utils/SPP3D.py:41-43) in one launch (ts_spp3d_pool_fwd); backward ts_spp3d_pool_bwd, a gather.
    `alias`: x is handed back as a second result; what flows into THAT (the concatenation's share of x's gradient) is added by the
    same backward launch instead of a pass of autograd's own."""

    @staticmethod
    def forward(ctx, x, strides, alias):
        _require_gpu(x)
        if x.dim() != 5:
            raise ValueError("spp3d_pool: x [B, C, D, H, W] (got %s)" % (tuple(x.shape),))
        x = _spp_dense(x)
        B, C, D, H, W = x.shape
        sizes = spp3d_level_sizes((D, H, W), strides)
        counts = [B * C * n[0] * n[1] * n[2] for n in sizes]
        pooled = torch.empty(sum(counts), device=x.device, dtype=torch.float32)
        s4 = strides + (0,) * (_SPP_MAX_LEVELS - len(strides))
        _lib.check(_lib.lib().ts_spp3d_pool_fwd(_lib.ptr(x), _lib.ptr(pooled), B, C, D, H, W, len(strides), s4[0], s4[1], s4[2], s4[3],
                                                x.stride(0), x.stride(1), _stream()), "ts_spp3d_pool_fwd")
        ctx.geom = (B, C, D, H, W, strides, s4, sizes, alias)
        outs, at = [], 0
        for n, cnt in zip(sizes, counts):
            outs.append(pooled[at:at + cnt].view(B, C, *n))
            at += cnt
        if alias:
            outs.append(x.view_as(x))
        return tuple(outs)

    @staticmethod
    def backward(ctx, *grads):
        B, C, D, H, W, strides, s4, sizes, alias = ctx.geom
        dev = next(g for g in grads if g is not None).device
        add = grads[len(strides)] if alias else None
        if add is not None:
            add = _spp_dense(add)
        gl = [g.contiguous() if g is not None else torch.zeros((B, C) + n, device=dev, dtype=torch.float32)
              for g, n in zip(grads[:len(strides)], sizes)]
        gl += [None] * (_SPP_MAX_LEVELS - len(gl))
        gx = torch.empty((B, C, D, H, W), device=dev, dtype=torch.float32)
        rc = _lib.lib().ts_spp3d_pool_bwd(_lib.ptr(gl[0]), _lib.ptr(gl[1]), _lib.ptr(gl[2]), _lib.ptr(gl[3]), _lib.ptr(add), _lib.ptr(gx),
                                          B, C, D, H, W, len(strides), s4[0], s4[1], s4[2], s4[3],
                                          add.stride(0) if add is not None else 0, add.stride(1) if add is not None else 0,
                                          gx.stride(0), gx.stride(1), _stream())
        _lib.check(rc, "ts_spp3d_pool_bwd")
        return gx, None, None


def spp3d_pool(x, strides, alias=False):
    """[avg_pool3d(x, k_s, k_s) for s in strides], k_s = (min(D,s), min(H,s), min(W,s)) (utils/SPP3D.py:41-43): one launch, the levels
    are views of one buffer.  alias=True appends x itself (see _Spp3dPool) -- hand THAT to spp3d_expand."""
    return list(_Spp3dPool.apply(x, _spp_strides(strides), bool(alias)))


class _Spp3dExpand(torch.autograd.Function):
    """cat([x] + [interpolate(l, (D,H,W), trilinear, align_corners=True) for l in levels], 1) (utils/SPP3D.py:45-47) in one launch;
    backward: the levels' gradients by ts_spp3d_expand_bwd (a gather per coarse cell), x's is a view of the incoming gradient."""

    @staticmethod
    def forward(ctx, x, strides, *levels):
        _require_gpu(x, *levels)
        x = _spp_dense(x)
        B, C, D, H, W = x.shape
        sizes = spp3d_level_sizes((D, H, W), strides)
        Cl = levels[0].shape[1]
        for l, n in zip(levels, sizes):
            if tuple(l.shape) != (B, Cl) + n:
                raise ValueError("spp3d_expand: level %s where %s is expected" % (tuple(l.shape), (B, Cl) + n))
        lv = [l.contiguous() for l in levels] + [None] * (_SPP_MAX_LEVELS - len(levels))
        cat = torch.empty((B, C + Cl * len(levels), D, H, W), device=x.device, dtype=torch.float32)
        s4 = strides + (0,) * (_SPP_MAX_LEVELS - len(strides))
        rc = _lib.lib().ts_spp3d_expand_fwd(_lib.ptr(x), _lib.ptr(lv[0]), _lib.ptr(lv[1]), _lib.ptr(lv[2]), _lib.ptr(lv[3]), _lib.ptr(cat),
                                            B, C, Cl, D, H, W, len(levels), s4[0], s4[1], s4[2], s4[3], x.stride(0), x.stride(1), _stream())
        _lib.check(rc, "ts_spp3d_expand_fwd")
        ctx.geom = (B, C, Cl, D, H, W, s4, sizes)
        return cat

    @staticmethod
    def backward(ctx, g):
        B, C, Cl, D, H, W, s4, sizes = ctx.geom
        g = _spp_dense(g)
        gl = [None] * _SPP_MAX_LEVELS
        if any(ctx.needs_input_grad[2:]):
            for i, n in enumerate(sizes):
                gl[i] = torch.empty((B, Cl) + n, device=g.device, dtype=torch.float32)
            rc = _lib.lib().ts_spp3d_expand_bwd(_lib.ptr(g), _lib.ptr(gl[0]), _lib.ptr(gl[1]), _lib.ptr(gl[2]), _lib.ptr(gl[3]), B, C, Cl, D, H, W,
                                                len(sizes), s4[0], s4[1], s4[2], s4[3], g.stride(0), g.stride(1), _stream())
            _lib.check(rc, "ts_spp3d_expand_bwd")
        return (g[:, :C] if ctx.needs_input_grad[0] else None, None) + tuple(gl[:len(sizes)])


def _spp_infer_strides(size, levels):
    """A stride per level that gives the level's size (the kernels describe a level by its stride; the resize only needs its size)."""
    out = []
    for l in levels:
        n = tuple(l.shape[2:])
        s = next((s for s in range(1, max(size) + 1) if spp3d_level_sizes(size, (s,))[0] == n), None)
        if s is None:
            raise ValueError("spp3d_expand: no stride pools %s to %s" % (tuple(size), n))
        out.append(s)
    return tuple(out)


def spp3d_expand(levels, x, strides=None):
    """cat([x, resize(levels[0]), ...], 1) with the trilinear align_corners resize of utils/SPP3D.py:45; `levels` as spp3d_pool(x,
    strides) lays them out (any channel count, the same for all).  Without `strides` they are inferred from the levels' sizes."""
    levels = list(levels)
    strides = _spp_strides(strides) if strides is not None else _spp_infer_strides(tuple(x.shape[2:]), levels)
    if len(levels) != len(strides):
        raise ValueError("spp3d_expand: %d levels for %d strides" % (len(levels), len(strides)))
    return _Spp3dExpand.apply(x, strides, *levels)


# --------------------------------------------------------------------------------------- element-wise glue of the levels
class _CandidatesInRange(torch.autograd.Function):
    """fine.py:82-93 / precise.py:73-78: the five candidates |high - low| * {0,3,4,5,8}/8 + min(low, high), behind the (detached)
    local-map candidates of the previous frames when there are any -- one launch each way instead of ~13 framework launches."""

    @staticmethod
    def forward(ctx, low, high, local_map):
        _require_gpu(low, high, local_map)
        low, high = _lib.contiguous(low), _lib.contiguous(high)
        B, _, H, W = low.shape
        nl = 0 if local_map is None else local_map.shape[1]
        out = torch.empty((B, nl + 5, H, W), device=low.device, dtype=torch.float32)
        L = _lib.lib()
        if nl:
            lm = _lib.contiguous(local_map)
            h, w = lm.shape[-2:]
            _lib.check(L.ts_resize_bilinear_fwd(_lib.ptr(lm), _lib.ptr(out), B, nl, h, w, H, W, float(W) / w, out.stride(0), _stream()),
                       "ts_resize_bilinear_fwd")
        _lib.check(L.ts_candidates_in_range_fwd(_lib.ptr(low), _lib.ptr(high), _lib.ptr(out), B, H, W, nl, nl + 5, _stream()),
                   "ts_candidates_in_range_fwd")
        ctx.save_for_backward(low, high)
        ctx.nl = nl
        return out

    @staticmethod
    def backward(ctx, g):
        low, high = ctx.saved_tensors
        B, _, H, W = low.shape
        g = _lib.contiguous(g)
        gl, gh = torch.empty_like(low), torch.empty_like(high)
        _lib.check(_lib.lib().ts_candidates_in_range_bwd(_lib.ptr(low), _lib.ptr(high), _lib.ptr(g), _lib.ptr(gl), _lib.ptr(gh), B, H, W,
                                                         ctx.nl, ctx.nl + 5, _stream()), "ts_candidates_in_range_bwd")
        return gl, gh, None


def candidates_in_range(low, high, local_map=None):
    """[B, n_local + 5, H, W]: `local_map` ([B, n_local, h, w], no gradient: the previous frames' state) resized to (H, W) with the
    disparity rescale of fine.py:89-93 in front of the five range candidates of fine.py:82-87."""
    if local_map is not None and local_map.requires_grad:
        raise NotImplementedError("candidates_in_range: the local map is temporal state and carries no gradient here")
    return _CandidatesInRange.apply(low, high, local_map)


class _OffsetHead(torch.autograd.Function):
    """PredictionHeads.regress_offset (module.py:384-390): tanh(x / 100).clamp(-1, 1) * delta, one launch each way."""

    @staticmethod
    def forward(ctx, x, delta):
        _require_gpu(x)
        x = _lib.contiguous(x)
        y = torch.empty_like(x)
        _lib.check(_lib.lib().ts_offset_head_fwd(_lib.ptr(x), _lib.ptr(y), x.numel(), float(delta), _stream()), "ts_offset_head_fwd")
        ctx.save_for_backward(x)
        ctx.delta = float(delta)
        return y

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        g = _lib.contiguous(g)
        gx = torch.empty_like(x)
        _lib.check(_lib.lib().ts_offset_head_bwd(_lib.ptr(x), _lib.ptr(g), _lib.ptr(gx), x.numel(), ctx.delta, _stream()), "ts_offset_head_bwd")
        return gx, None


def offset_head(x, delta):
    return _OffsetHead.apply(x, delta)


# --------------------------------------------------------------------------------------- K3 element stages
class _ResizeAddSiLU(torch.autograd.Function):
    """silu(F.interpolate(a, size, 'trilinear', align_corners=True) + add): ResidualBlock3D up-steps
    (module.py:285-295) as one kernel each way (ts_resize3d_add_act_{fwd,bwd})."""

    @staticmethod
    def forward(ctx, a, add):
        _require_gpu(a, add)
        a, add = a.contiguous(), add.contiguous()
        B, C, Da, Ha, Wa = a.shape
        D, H, W = add.shape[2:]
        out = torch.empty_like(add)
        na, n = Da * Ha * Wa, D * H * W
        rc = _lib.lib().ts_resize3d_add_act_fwd(_lib.ptr(a), _lib.ptr(add), _lib.ptr(out), B, C, Da, Ha, Wa, D, H, W, 1,
                                                C * na, na, C * n, n, C * n, n, _stream())
        _lib.check(rc, "ts_resize3d_add_act_fwd")
        ctx.save_for_backward(a, add)
        return out

    @staticmethod
    def backward(ctx, g):
        a, add = ctx.saved_tensors
        B, C, Da, Ha, Wa = a.shape
        D, H, W = add.shape[2:]
        g = g.contiguous()
        ga, gadd = torch.empty_like(a), torch.empty_like(add)
        rc = _lib.lib().ts_resize3d_add_act_bwd(_lib.ptr(a), _lib.ptr(add), _lib.ptr(g), _lib.ptr(ga), _lib.ptr(gadd),
                                                B, C, Da, Ha, Wa, D, H, W, 1, _stream())
        _lib.check(rc, "ts_resize3d_add_act_bwd")
        return ga, gadd


def resize_add_silu(a, add):
    """F.silu(F.interpolate(a, size=add.shape[-3:], mode='trilinear', align_corners=True) + add)."""
    return _ResizeAddSiLU.apply(a, add)


class _Pool5AvgMax(torch.autograd.Function):
    """(avg_pool3d, max_pool3d)(x, kernel 5, stride 1, padding 2) of PyramidFusion (module.py:415-417)."""

    @staticmethod
    def forward(ctx, x):
        _require_gpu(x)
        x = x.contiguous()
        B, C, D, H, W = x.shape
        if min(D, H, W) < 5:      # what F.avg_pool3d(kernel 5) answers, padding or not (PyramidFusion, module.py:416)
            raise RuntimeError("input image (T: %d H: %d W: %d) smaller than kernel size (kT: 5 kH: 5 kW: 5)" % (D, H, W))
        avg, mx = torch.empty_like(x), torch.empty_like(x)
        n = D * H * W
        rc = _lib.lib().ts_pool3d5_avgmax_fwd(_lib.ptr(x), _lib.ptr(avg), _lib.ptr(mx), B, C, D, H, W,
                                              C * n, n, C * n, n, C * n, n, _stream())
        _lib.check(rc, "ts_pool3d5_avgmax_fwd")
        ctx.save_for_backward(x)
        return avg, mx

    @staticmethod
    def backward(ctx, g_avg, g_max):
        (x,) = ctx.saved_tensors
        B, C, D, H, W = x.shape
        gx = torch.empty_like(x)
        # Named references, not temporaries: under torch.cat the two gradients arrive as channel slices, `.contiguous()` makes copies,
        # and a copy that is only alive inside `_lib.ptr(...)` hands its block back to the allocator before the next argument is
        # evaluated -- the second copy then lands in the SAME block and the kernel reads dMax through both pointers (round 3: the
        # composed backward was 2-6 % off below every PyramidFusion while each per-op test, fed contiguous gradients, was green).
        g_avg, g_max = g_avg.contiguous(), g_max.contiguous()
        rc = _lib.lib().ts_pool3d5_avgmax_bwd(_lib.ptr(x), _lib.ptr(g_avg), _lib.ptr(g_max),
                                              _lib.ptr(gx), B, C, D, H, W, _stream())
        _lib.check(rc, "ts_pool3d5_avgmax_bwd")
        return gx


def pool5_avgmax(x):
    """(F.avg_pool3d(x, 5, 1, 2), F.max_pool3d(x, 5, 1, 2)) in one pass over x."""
    return _Pool5AvgMax.apply(x)


class _SortGather(torch.autograd.Function):
    """disp_sample, order = sort(disp_sample, dim=1, stable); volume = gather(volume, dim=2, order)
    (coarse.py:103-105, fine.py:120-122) as one kernel each way."""

    @staticmethod
    def forward(ctx, volume, sample):
        _require_gpu(volume, sample)
        volume, sample = volume.contiguous(), sample.contiguous()
        B, C, DT, H, W = volume.shape
        out_v, out_s = torch.empty_like(volume), torch.empty_like(sample)
        n = DT * H * W
        rc = _lib.lib().ts_merge_candidates_fwd(_lib.ptr(volume), _lib.ptr(sample), None, None, None, None, None,
                                                _lib.ptr(out_s), _lib.ptr(out_v), B, C, DT, 0, H, W, C * n, n, C * n, n, _stream())
        _lib.check(rc, "ts_merge_candidates_fwd")
        ctx.save_for_backward(sample)
        return out_v, out_s

    @staticmethod
    def backward(ctx, g_v, g_s):
        (sample,) = ctx.saved_tensors
        B, DT, H, W = sample.shape
        g_v = g_v.contiguous()
        g_s = g_s.contiguous() if g_s is not None else None
        C = g_v.shape[1]
        gv, gs = torch.empty_like(g_v), torch.empty_like(sample)
        rc = _lib.lib().ts_merge_candidates_bwd(_lib.ptr(sample), _lib.ptr(g_v), _lib.ptr(g_s),
                                                _lib.ptr(gv), _lib.ptr(gs), B, C, DT, H, W, _stream())
        _lib.check(rc, "ts_merge_candidates_bwd")
        return gv, gs


def sort_gather(volume, sample):
    """-> (volume permuted along D by the stable ascending order of `sample`, sorted sample)."""
    return _SortGather.apply(volume, sample)


def block_cost_warped(reference_fm, target_fm, disp_sample, block_cost_scale=3):
    """Inference form of the sampled block_cost WITHOUT its first C channels (the D-fold repeat of
    reference_fm, block_cost.py:51): [B, C + scales*C/8, D, H, W].  No autograd.  Used with the
    `addend` of ts_conv3d_hw_fwd, see include/ts_hip.h."""
    _require_gpu(reference_fm, target_fm, disp_sample)
    left, right, disp = _lib.contiguous(reference_fm), _lib.contiguous(target_fm), _lib.contiguous(disp_sample)
    B, C, H, W = left.shape
    D = disp.shape[1]
    if C % 8 != 0:
        raise ValueError("channel count must be a multiple of 8 (block_cost.py:9)")
    L = _lib.lib()
    out = torch.empty((B, C + block_cost_scale * (C // 8), D, H, W), device=left.device, dtype=torch.float32)
    ws = torch.empty(max(int(L.ts_block_cost_workspace_bytes(B, C, H, W, D, block_cost_scale)), 256),
                     device=left.device, dtype=torch.uint8)

    def launch():
        return L.ts_block_cost_sampled_warped_fwd(_lib.ptr(left), _lib.ptr(right), _lib.ptr(disp), _lib.ptr(out),
                                                  _lib.ptr(ws), B, C, H, W, D, block_cost_scale, _stream())
    rc = launch() if _k1_probe is None else _k1_probe((B, C, H, W, D, "warped"), launch)
    _lib.check(rc, "ts_block_cost_sampled_warped_fwd")
    return out


class _BlockCostWarped(torch.autograd.Function):
    """The sampled block_cost WITHOUT its first C channels (block_cost_warped) with autograd: ts_block_cost_sampled_warped_{fwd,bwd}.
    The training path's first layer of a sampled level takes the D-invariant left half as a per-pixel term (first_layer_split)."""

    @staticmethod
    def forward(ctx, left, right, disp, scales):
        out = block_cost_warped(left, right, disp, scales)
        ctx.save_for_backward(_lib.contiguous(left), _lib.contiguous(right), _lib.contiguous(disp))
        ctx.scales = int(scales)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        left, right, disp = ctx.saved_tensors
        B, C, H, W = left.shape
        D, scales = disp.shape[1], ctx.scales
        L = _lib.lib()
        grad_out = _lib.contiguous(grad_out)
        gl = torch.empty_like(left) if ctx.needs_input_grad[0] else None
        gr = torch.empty_like(right) if ctx.needs_input_grad[1] else None
        gd = torch.empty_like(disp) if ctx.needs_input_grad[2] else None
        ws = torch.empty(max(int(L.ts_block_cost_bwd_workspace_bytes(B, C, H, W, D, scales)), 256), device=left.device, dtype=torch.uint8)
        _lib.check(L.ts_block_cost_sampled_warped_bwd(_lib.ptr(left), _lib.ptr(right), _lib.ptr(disp), _lib.ptr(grad_out), _lib.ptr(gl),
                                                      _lib.ptr(gr), _lib.ptr(gd), _lib.ptr(ws), B, C, H, W, D, scales, _stream()),
                   "ts_block_cost_sampled_warped_bwd")
        return gl, gr, gd, None


class _SplitWeight(torch.autograd.Function):
    """weight [Cout, Cin, ...] -> (weight[:, :n], weight[:, n:]) as CONTIGUOUS tensors; backward: one concatenation."""

    @staticmethod
    def forward(ctx, weight, n):
        ctx.n = int(n)
        return weight[:, :n].contiguous(), weight[:, n:].contiguous()

    @staticmethod
    def backward(ctx, g1, g2):
        return torch.cat([g1, g2], dim=1), None


def first_layer_split(conv, left, volume):
    """The (1,3,3) convolution + BatchNorm + activation over a sampled level's volume [left x D | warped right | corr]
    (precise.py:88-91, fine.py:96-103 over block_cost.py:47-58) WITHOUT the left half in the volume: its channels are the left features
    repeated over the D candidates (block_cost.py:51), so their share of the layer is a 2-D convolution of `left`, computed once per
    pixel and added to every depth plane before the bias / BatchNorm -- in training as the inference engine has done since round 1.
    `conv`: the layers.Conv3d wrapper (its weight covers all 2C + scales*C/8 input channels); `volume` = block_cost_warped_ag(...):
    [B, C + scales*C/8, D, H, W].  The layer's forward reads 42 % fewer channels, its input gradient and weight gradient likewise, the
    cost volume's backward receives no gradient for the half that is not there; the left term's own backward is two single-plane
    launches on the sum over D of the layer's output gradient."""
    C = left.shape[1]
    w1, w2 = _SplitWeight.apply(conv._parameters["weight"], C)
    dil = conv.dilation[1]
    lt = _ConvRaw.apply(left.unsqueeze(2), w1, None, "hw", (1, dil, False))     # [B, Cout, 1, H, W], raw
    act = conv._fusable()
    if act is False or conv.stride[1] != 1:
        raise NotImplementedError("first_layer_split: a stride-1 (1,3,3) convolution + BatchNorm (+ SiLU / ReLU)")
    if _WGRAD_DEFER is not None:
        _WGRAD_DEFER.used(w2)               # its gradient is concatenated with w1's DURING backward: never a deferred finish (counts as shared)
    return conv_bn_act(volume, w2, conv._parameters["bias"], conv._modules["norm"], act, "hw", (1, dil, False), addend=lt)


def block_cost_warped_ag(reference_fm, target_fm, disp_sample, block_cost_scale=3):
    return _BlockCostWarped.apply(reference_fm, target_fm, disp_sample, int(block_cost_scale))


class Split:
    """An input whose channels live in two allocations: `a` holds channels [0, Ca), `b` the rest.  block_cost_corr and the native
    pipeline's conv_hw / conv_d read it in place through the ts_*_split_fwd entries (include/ts_hip.h) -- bit-identical to the
    plain entry on torch.cat([a, b], 1).  shape / detach / contiguous / repeat: what a caller that only inspects or keeps its
    arguments needs; contiguous() and repeat() MAKE the concatenation (a framework copy: diagnostics and measurements, never part
    of a pass)."""
    __slots__ = ("a", "b")

    def __init__(self, a, b):
        if a.shape[0] != b.shape[0] or a.shape[2:] != b.shape[2:]:
            raise ValueError("Split: the two parts differ outside the channel axis: %r, %r" % (tuple(a.shape), tuple(b.shape)))
        self.a, self.b = a, b

    device = property(lambda self: self.a.device)
    shape = property(lambda self: (self.a.shape[0], self.a.shape[1] + self.b.shape[1]) + tuple(self.a.shape[2:]))

    def unsqueeze(self, dim):
        return Split(self.a.unsqueeze(dim), self.b.unsqueeze(dim))

    def detach(self):
        return Split(self.a.detach(), self.b.detach())

    def cat(self):
        return torch.cat([self.a, self.b], 1)

    def contiguous(self):
        return self.cat()

    def repeat(self, *sizes):
        return self.cat().repeat(*sizes)


def block_cost_corr(reference_fm, target_fm, disp_sample, block_cost_scale=3):
    """Inference form of the sampled block_cost WITHOUT its 2C main channels: the correlation blocks alone,
    [B, scales*C/8, D, H, W] = block_cost(...)[:, 2C:].  No autograd.  The consumer is ts_conv3d_hw_warp_fwd, which takes the
    warped half of the volume in pre-contracted form (include/ts_hip.h).
    The two maps may be Splits at the same channel: the result is that of their concatenations, which are never made
    (ts_block_cost_sampled_corr_split_fwd); dense planes, any batch stride."""
    if isinstance(reference_fm, Split) or isinstance(target_fm, Split):
        if not (isinstance(reference_fm, Split) and isinstance(target_fm, Split)) or reference_fm.a.shape[1] != target_fm.a.shape[1]:
            raise ValueError("block_cost_corr: both maps split at the same channel, or neither")
        _require_gpu(reference_fm.a, target_fm.a, disp_sample)
        return _block_cost_corr_split(reference_fm.a, reference_fm.b, target_fm.a, target_fm.b, _lib.contiguous(disp_sample),
                                      block_cost_scale)
    _require_gpu(reference_fm, target_fm, disp_sample)
    left, right, disp = _lib.contiguous(reference_fm), _lib.contiguous(target_fm), _lib.contiguous(disp_sample)
    B, C, H, W = left.shape
    D = disp.shape[1]
    if C % 8 != 0:
        raise ValueError("channel count must be a multiple of 8 (block_cost.py:9)")
    L = _lib.lib()
    out = torch.empty((B, block_cost_scale * (C // 8), D, H, W), device=left.device, dtype=torch.float32)
    ws = torch.empty(max(_q("ts_block_cost_workspace_bytes", B, C, H, W, D, block_cost_scale), 256), device=left.device, dtype=torch.uint8)

    def launch():
        return L.ts_block_cost_sampled_corr_fwd(_lib.ptr(left), _lib.ptr(right), _lib.ptr(disp), _lib.ptr(out),
                                                _lib.ptr(ws), B, C, H, W, D, block_cost_scale, _stream())
    rc = launch() if _k1_probe is None else _k1_probe((B, C, H, W, D, "corr"), launch)
    _lib.check(rc, "ts_block_cost_sampled_corr_fwd")
    return out


def _block_cost_corr_split(left, left2, right, right2, disp, scales):
    _require_gpu(left2, right2)
    B, Cs, H, W = left.shape
    C = Cs + left2.shape[1]
    D = disp.shape[1]
    for t, c in ((left, Cs), (right, Cs), (left2, C - Cs), (right2, C - Cs)):
        if tuple(t.shape) != (B, c, H, W) or t.stride(3) != 1 or t.stride(2) != W or t.stride(1) != H * W:
            raise ValueError("block_cost_corr: split maps need one geometry and dense planes, got %r strides %r" % (tuple(t.shape), t.stride()))
    L = _lib.lib()
    out = torch.empty((B, scales * (C // 8), D, H, W), device=left.device, dtype=torch.float32)
    ws = torch.empty(max(_q("ts_block_cost_workspace_bytes", B, C, H, W, D, scales), 256), device=left.device, dtype=torch.uint8)

    def launch():
        return L.ts_block_cost_sampled_corr_split_fwd(_lib.ptr(left), _lib.ptr(left2), _lib.ptr(right), _lib.ptr(right2), _lib.ptr(disp),
                                                      _lib.ptr(out), _lib.ptr(ws), B, C, Cs, H, W, D, scales, left.stride(0),
                                                      left2.stride(0), right.stride(0), right2.stride(0), _stream())
    rc = launch() if _k1_probe is None else _k1_probe((B, C, H, W, D, "corr"), launch)
    _lib.check(rc, "ts_block_cost_sampled_corr_split_fwd")
    return out


def block_cost(reference_fm, target_fm, disp_sample, block_cost_scale=3):
    """Cost volume of `block_cost` (block_cost.py:16-83), same arguments and output layout.

    disp_sample: int -> integer candidates 0..D-1 (out [B, C+s*C/8, D, H, W]);
                 Tensor [B,D,H,W] -> per-pixel candidates (out [B, 2C+s*C/8, D, H, W]).
    """
    scales = int(block_cost_scale)
    if isinstance(disp_sample, int):
        return _BlockCost.apply(reference_fm, target_fm, None, disp_sample, scales)
    return _BlockCost.apply(reference_fm, target_fm, disp_sample, 0, scales)


# --------------------------------------------------------------------------------------------- K5 (training form)
class _ConvexUpsample(torch.autograd.Function):
    """ConvexUpsample's combination step (module.py:337-353): softmax over the k*k logits of every output pixel, weighted sum of
    the 3x3 neighbourhood of `disp * scale`.  logits [B, 9*r*r, H, W], disp [B,1,H,W] -> [B,1,H*r,W*r]."""

    @staticmethod
    def forward(ctx, logits, disp, r, scale):
        _require_gpu(logits, disp)
        logits, disp = _lib.contiguous(logits), _lib.contiguous(disp)
        B, _, H, W = disp.shape
        if logits.shape[1] != 9 * r * r or disp.shape[1] != 1:
            raise ValueError("convex upsample: logits must be [B, 9*r*r, H, W] and disp [B,1,H,W]")
        out = torch.empty((B, 1, H * r, W * r), device=disp.device, dtype=torch.float32)
        _lib.check(_lib.lib().ts_convex_upsample_fwd(_lib.ptr(logits), _lib.ptr(disp), _lib.ptr(out), B, H, W, r, float(scale), _stream()),
                   "ts_convex_upsample_fwd")
        ctx.save_for_backward(logits, disp)
        ctx.meta = (r, float(scale))
        return out

    @staticmethod
    def backward(ctx, g):
        logits, disp = ctx.saved_tensors
        r, scale = ctx.meta
        B, _, H, W = disp.shape
        gl = torch.empty_like(logits) if ctx.needs_input_grad[0] else None
        gd = torch.empty_like(disp) if ctx.needs_input_grad[1] else None
        g = _lib.contiguous(g)
        _lib.check(_lib.lib().ts_convex_upsample_bwd(_lib.ptr(logits), _lib.ptr(disp), _lib.ptr(g), _lib.ptr(gl), _lib.ptr(gd),
                                                     B, H, W, r, scale, _stream()), "ts_convex_upsample_bwd")
        return gl, gd, None, None


def convex_upsample(logits, disp, upscale_factor, disp_scale):
    return _ConvexUpsample.apply(logits, disp, int(upscale_factor), float(disp_scale))


class _UNetUpsample(torch.autograd.Function):
    """UNet.upsample (module.py:468-482): softmax over the 9 logit planes, bilinear (align_corners) upsampling of the unfolded
    disparity * Wo / w, weighted sum.  logits [B,9,Ho,Wo], disp [B,1,h,w] -> [B,1,Ho,Wo]."""

    @staticmethod
    def forward(ctx, logits, disp):
        _require_gpu(logits, disp)
        logits, disp = _lib.contiguous(logits), _lib.contiguous(disp)
        B, _, Ho, Wo = logits.shape
        h, w = disp.shape[-2:]
        out = torch.empty((B, 1, Ho, Wo), device=disp.device, dtype=torch.float32)
        _lib.check(_lib.lib().ts_unet_upsample_fwd(_lib.ptr(logits), _lib.ptr(disp), _lib.ptr(out), B, h, w, Ho, Wo, _stream()),
                   "ts_unet_upsample_fwd")
        ctx.save_for_backward(logits, disp)
        return out

    @staticmethod
    def backward(ctx, g):
        logits, disp = ctx.saved_tensors
        B, _, Ho, Wo = logits.shape
        h, w = disp.shape[-2:]
        gl = torch.empty_like(logits)
        gd = torch.empty_like(disp) if ctx.needs_input_grad[1] else None
        ws = torch.empty_like(logits)
        g = _lib.contiguous(g)
        _lib.check(_lib.lib().ts_unet_upsample_bwd(_lib.ptr(logits), _lib.ptr(disp), _lib.ptr(g), _lib.ptr(gl), _lib.ptr(gd),
                                                   _lib.ptr(ws), B, h, w, Ho, Wo, _stream()), "ts_unet_upsample_bwd")
        return gl, gd


def unet_upsample(logits, disp):
    return _UNetUpsample.apply(logits, disp)


class _ResizePair(torch.autograd.Function):
    """(F.interpolate(x0 * s0, size), F.interpolate(x1 * s1, size)), bilinear, align_corners=True, in one launch
    (ts_resize_bilinear_pair_fwd): the top-k memory's candidates and costs (precise.py:100-103, coarse.py:91-96).  The memory is
    temporal state -- nothing in a training step differentiates it -- so the backward (the framework's own adjoint, recomputed)
    exists for completeness."""

    @staticmethod
    def forward(ctx, x0, x1, H, W, s0, s1):
        _require_gpu(x0, x1)
        a, b = _lib.contiguous(x0), _lib.contiguous(x1)
        if a.shape != b.shape or a.dim() != 4:
            raise ValueError("resize_bilinear_pair: two [B,C,h,w] maps of one shape")
        B, C, h, w = a.shape
        o0 = torch.empty((B, C, H, W), device=a.device, dtype=torch.float32)
        o1 = torch.empty_like(o0)
        _lib.check(_lib.lib().ts_resize_bilinear_pair_fwd(_lib.ptr(a), _lib.ptr(b), _lib.ptr(o0), _lib.ptr(o1), B, C, h, w, H, W,
                                                          float(s0), float(s1), _stream()), "ts_resize_bilinear_pair_fwd")
        ctx.meta = (tuple(a.shape), H, W, float(s0), float(s1))
        ctx.set_materialize_grads(False)
        return o0, o1

    @staticmethod
    def backward(ctx, g0, g1):
        shape, H, W, s0, s1 = ctx.meta
        outs = []
        for g, sc in ((g0, s0), (g1, s1)):
            if g is None:
                outs.append(None)
                continue
            with torch.enable_grad():
                x = torch.zeros(shape, device=g.device, dtype=g.dtype, requires_grad=True)
                y = torch.nn.functional.interpolate(x * sc, size=(H, W), mode="bilinear", align_corners=True)
            outs.append(torch.autograd.grad(y, x, g)[0])
        return outs[0], outs[1], None, None, None, None


def resize_bilinear_pair(x0, x1, size, scale0=1.0, scale1=1.0):
    return _ResizePair.apply(x0, x1, int(size[0]), int(size[1]), float(scale0), float(scale1))


_CONST = {}


def const_zeros(shape, device):
    """A shared all-zero tensor (READ-ONLY by contract: the absent cost memory of a first frame) instead of a fill launch per call."""
    key = ("z", tuple(shape), device)
    if key not in _CONST:
        if torch.cuda.is_current_stream_capturing():       # a capture's allocations belong to its pool: nothing of them is kept
            return torch.zeros(shape, device=device, dtype=torch.float32)
        _CONST[key] = torch.zeros(shape, device=device, dtype=torch.float32)
    return _CONST[key]


def const_arange(n, device):
    key = ("a", int(n), device)
    if key not in _CONST:
        if torch.cuda.is_current_stream_capturing():
            return torch.arange(n, device=device, dtype=torch.float32)
        _CONST[key] = torch.arange(n, device=device, dtype=torch.float32)
    return _CONST[key]


class _WeightedTotal(torch.autograd.Function):
    """sum_i w_i * term_i of 0-d loss terms: one stack + one dot product forward, one multiplication backward (the framework's
    form -- a multiplication per term each way, a stack and a sum -- was ~25 one-element launches per training step)."""

    @staticmethod
    def forward(ctx, wvec, *terms):
        ctx.save_for_backward(wvec)
        return torch.dot(torch.stack([t.reshape(()) for t in terms]), wvec)

    @staticmethod
    def backward(ctx, g):
        (wvec,) = ctx.saved_tensors
        gv = wvec * g
        return (None,) + tuple(gv.unbind(0))


_WVEC = {}


def weighted_total(terms, weights):
    """sum_i weights[i] * terms[i] (0-d tensors; weights: python floats)."""
    key = (tuple(float(w) for w in weights), terms[0].device)
    if key not in _WVEC:
        _WVEC[key] = torch.tensor(key[0], device=terms[0].device, dtype=torch.float32)
    return _WeightedTotal.apply(_WVEC[key], *terms)


# --------------------------------------------------------------------------------------------- K4
class _TopkSoftArgmax(torch.autograd.Function):
    """K4a.  ts_topk_softargmax_{fwd,bwd}; returns (disp, topk_disp, topk_cost)."""

    @staticmethod
    def forward(ctx, cost, sample, offset, k):
        _require_gpu(cost, sample, offset)
        if cost.dim() != 4 or cost.shape != sample.shape or cost.shape != offset.shape:
            raise ValueError("cost, disp_sample and off must be [B,D,H,W] of equal shape")
        cost, sample, offset = _lib.contiguous(cost), _lib.contiguous(sample), _lib.contiguous(offset)
        B, D, H, W = cost.shape
        disp = torch.empty((B, 1, H, W), device=cost.device, dtype=torch.float32)
        tdisp = torch.empty((B, k, H, W), device=cost.device, dtype=torch.float32)
        tcost = torch.empty_like(tdisp)
        tidx = torch.empty((B, k, H, W), device=cost.device, dtype=torch.int32)
        rc = _lib.lib().ts_topk_softargmax_fwd(_lib.ptr(cost), _lib.ptr(sample), _lib.ptr(offset), _lib.ptr(disp),
                                               _lib.ptr(tdisp), _lib.ptr(tcost), _lib.ptr(tidx), B, D, H, W, int(k),
                                               _stream())
        _lib.check(rc, "ts_topk_softargmax_fwd")
        ctx.save_for_backward(tdisp, tcost, tidx, disp)
        ctx.meta = (B, D, H, W, int(k))
        ctx.set_materialize_grads(False)         # unused outputs (the top-k planes when nothing differentiates the memory) arrive as None,
        return disp, tdisp, tcost                # which the kernel takes as NULL: no zero-fill launches

    @staticmethod
    def backward(ctx, g_disp, g_tdisp, g_tcost):
        tdisp, tcost, tidx, disp = ctx.saved_tensors
        B, D, H, W, k = ctx.meta
        need_cost = ctx.needs_input_grad[0]
        need_samp = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        gcost = torch.empty((B, D, H, W), device=disp.device, dtype=torch.float32) if need_cost else None
        gsamp = torch.empty((B, D, H, W), device=disp.device, dtype=torch.float32) if need_samp else None
        c = lambda t: None if t is None else _lib.contiguous(t)
        rc = _lib.lib().ts_topk_softargmax_bwd(_lib.ptr(tdisp), _lib.ptr(tcost), _lib.ptr(tidx), _lib.ptr(disp),
                                               _lib.ptr(c(g_disp)), _lib.ptr(c(g_tdisp)), _lib.ptr(c(g_tcost)),
                                               _lib.ptr(gcost), _lib.ptr(gsamp), B, D, H, W, k, _stream())
        _lib.check(rc, "ts_topk_softargmax_bwd")
        return (gcost, gsamp if ctx.needs_input_grad[1] else None,
                gsamp if ctx.needs_input_grad[2] else None, None)


def topk_softargmax(cost, disp_sample, off, k=2):
    """predict_disp() of the reference levels (coarse.py:69-75): (disp_map, topk_disp, topk_cost)."""
    return _TopkSoftArgmax.apply(cost, disp_sample, off, int(k))


class _SoftArgmin(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cost, sample, temperature, normalize):
        _require_gpu(cost, sample)
        cost, sample = _lib.contiguous(cost), _lib.contiguous(sample)
        B, D, H, W = cost.shape
        disp = torch.empty((B, 1, H, W), device=cost.device, dtype=torch.float32)
        rc = _lib.lib().ts_softargmin_fwd(_lib.ptr(cost), _lib.ptr(sample), _lib.ptr(disp), float(temperature),
                                          int(bool(normalize)), B, D, H, W, _stream())
        _lib.check(rc, "ts_softargmin_fwd")
        ctx.save_for_backward(cost, sample, disp)
        ctx.meta = (B, D, H, W, float(temperature), int(bool(normalize)))
        return disp

    @staticmethod
    def backward(ctx, g):
        cost, sample, disp = ctx.saved_tensors
        B, D, H, W, temperature, normalize = ctx.meta
        gc = torch.empty_like(cost) if ctx.needs_input_grad[0] else None
        gs = torch.empty_like(sample) if ctx.needs_input_grad[1] else None
        g = _lib.contiguous(g)
        rc = _lib.lib().ts_softargmin_bwd(_lib.ptr(cost), _lib.ptr(sample), _lib.ptr(disp), _lib.ptr(g),
                                          _lib.ptr(gc), _lib.ptr(gs), temperature, normalize, B, D, H, W, _stream())
        _lib.check(rc, "ts_softargmin_bwd")
        return gc, gs, None, None


def soft_argmin(cost_volume, disp_sample, temperature=1.0, normalize=True):
    """SOFTARGMIN.forward (prediction/soft_argmin.py:38-59)."""
    if cost_volume.dim() != 4:
        raise ValueError('expected 4D input (got {}D input)'.format(cost_volume.dim()))
    if cost_volume.shape != disp_sample.shape:
        raise ValueError('The shape of disparity samples and cost volume should be consistent!')
    return _SoftArgmin.apply(cost_volume, disp_sample, temperature, normalize)


class _ArgmaxSelect(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cost, sample):
        _require_gpu(cost, sample)
        cost, sample = _lib.contiguous(cost), _lib.contiguous(sample)
        B, D, H, W = cost.shape
        disp = torch.empty((B, 1, H, W), device=cost.device, dtype=torch.float32)
        idx = torch.empty((B, 1, H, W), device=cost.device, dtype=torch.int32)
        rc = _lib.lib().ts_argmax_select_fwd(_lib.ptr(cost), _lib.ptr(sample), _lib.ptr(disp), _lib.ptr(idx),
                                             B, D, H, W, _stream())
        _lib.check(rc, "ts_argmax_select_fwd")
        ctx.save_for_backward(idx)
        ctx.shape = sample.shape
        return disp

    @staticmethod
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        gs = torch.zeros(ctx.shape, device=g.device, dtype=g.dtype)
        gs.scatter_(1, idx.long(), g)          # index plumbing only; one element per pixel
        return None, gs


def argmin_select(cost_volume, disp_sample):
    """ARGMIN.forward (prediction/argmin.py:35-46): gather the sample of the best (max) cost."""
    if cost_volume.shape != disp_sample.shape:
        raise ValueError("{}, {}".format(cost_volume.shape, disp_sample.shape))
    return _ArgmaxSelect.apply(cost_volume, disp_sample)


# --------------------------------------------------------------------------------------------- K2
class _SplatSum(torch.autograd.Function):
    """_FunctionSoftsplat of the reference (softsplat.py:239-332) on ts_softsplat_sum_*."""

    @staticmethod
    def forward(ctx, inp, flow, deterministic=False):
        _require_gpu(inp, flow)
        if flow.shape[1] != 2 or inp.shape[0] != flow.shape[0] or inp.shape[2:] != flow.shape[2:]:
            raise ValueError("flow must be [B,2,H,W] matching the input")
        inp, flow = _lib.contiguous(inp), _lib.contiguous(flow)
        B, C, H, W = inp.shape
        out = torch.empty_like(inp)
        if deterministic:      # 64-bit fixed-point accumulation: the same bits every run
            ws = torch.empty(B * C * H * W * 8, device=inp.device, dtype=torch.uint8)
            _lib.check(_lib.lib().ts_softsplat_sum_fwd_deterministic(_lib.ptr(inp), _lib.ptr(flow), _lib.ptr(out), _lib.ptr(ws),
                                                                     B, C, H, W, _stream()), "ts_softsplat_sum_fwd_deterministic")
        else:
            _lib.check(_lib.lib().ts_softsplat_sum_fwd(_lib.ptr(inp), _lib.ptr(flow), _lib.ptr(out), B, C, H, W, _stream()),
                       "ts_softsplat_sum_fwd")
        ctx.save_for_backward(inp, flow)
        return out

    @staticmethod
    def backward(ctx, g):
        inp, flow = ctx.saved_tensors
        B, C, H, W = inp.shape
        g = _lib.contiguous(g)
        gi = gf = None
        if ctx.needs_input_grad[0]:
            gi = torch.empty_like(inp)
            _lib.check(_lib.lib().ts_softsplat_sum_bwd_input(_lib.ptr(flow), _lib.ptr(g), _lib.ptr(gi), B, C, H, W,
                                                             _stream()), "ts_softsplat_sum_bwd_input")
        if ctx.needs_input_grad[1]:
            gf = torch.empty_like(flow)
            _lib.check(_lib.lib().ts_softsplat_sum_bwd_flow(_lib.ptr(inp), _lib.ptr(flow), _lib.ptr(g), _lib.ptr(gf),
                                                            B, C, H, W, _stream()), "ts_softsplat_sum_bwd_flow")
        return gi, gf, None


def FunctionSoftsplat(tenInput, tenFlow, tenMetric, strType, deterministic=False):
    """Forward splatting, same signature as the reference's FunctionSoftsplat (softsplat.py:334-360).
    deterministic=True (an addition): order-independent accumulation, bit-identical from run to run.

    'softmax' on inputs that do not require grad (the only use in update_map) runs the fused kernel
    ts_softsplat_softmax_fwd; every other case composes the summation splat (with HIP backward)."""
    if tenMetric is not None and tenMetric.shape[1] != 1:
        raise ValueError("tenMetric must have one channel")
    if strType not in ('summation', 'average', 'linear', 'softmax'):
        raise ValueError("unknown splatting type %r" % (strType,))
    grad_needed = torch.is_grad_enabled() and any(
        t is not None and t.requires_grad for t in (tenInput, tenFlow, tenMetric))
    if strType == 'softmax' and not grad_needed and not deterministic:
        _require_gpu(tenInput, tenFlow, tenMetric)
        inp, flow, met = _lib.contiguous(tenInput), _lib.contiguous(tenFlow), _lib.contiguous(tenMetric)
        B, C, H, W = inp.shape
        L = _lib.lib()
        out = torch.empty_like(inp)
        ws = torch.empty(int(L.ts_softsplat_softmax_workspace_bytes(B, C, H, W)), device=inp.device, dtype=torch.uint8)
        _lib.check(L.ts_softsplat_softmax_fwd(_lib.ptr(inp), _lib.ptr(flow), _lib.ptr(met), _lib.ptr(out), _lib.ptr(ws),
                                              B, C, H, W, _stream()), "ts_softsplat_softmax_fwd")
        return out
    x = tenInput
    if strType == 'average':
        x = torch.cat([x, x.new_ones(x.shape[0], 1, x.shape[2], x.shape[3])], 1)
    elif strType == 'linear':
        x = torch.cat([x * tenMetric, tenMetric], 1)
    elif strType == 'softmax':
        e = tenMetric.exp()
        x = torch.cat([x * e, e], 1)
    out = _SplatSum.apply(x, tenFlow, deterministic)
    if strType != 'summation':
        out = out[:, :-1, :, :] / (out[:, -1:, :, :] + 1e-22)
    return out


def reproject_memory(prev_disp, mem_disp, mem_cost, local_map, n_local_out, K, T_a, T_b, baseline, factor, h, w):
    """The fused temporal state update (ts_reproject_memory_fwd): what update_past_cost and update_local_map of
    the reference (projects/TemporalStereo/TemporalStereo.py:386-426, :340-384) compute together, three launches.

    prev_disp [B,1,H,W]; mem_disp/mem_cost [B,k,h,w] or None; local_map [B,n,h,w] or None; K [B,3|4,3|4] full-
    resolution intrinsics; T = T_a @ T_b (T_b may be None); baseline scalar or tensor with B elements.
    Returns (moved mem_disp, moved mem_cost, moved local map), None where not requested."""
    _require_gpu(prev_disp, K, T_a)
    if prev_disp.dim() != 4 or prev_disp.shape[1] != 1:
        raise RuntimeError("reproject_memory: prev_disp must be [B,1,H,W], got %s" % (tuple(prev_disp.shape),))
    B, _, Hf, Wf = prev_disp.shape
    dev = prev_disp.device
    prev_disp = _lib.contiguous(prev_disp)
    k = 0
    if mem_disp is not None:
        mem_disp, mem_cost = _lib.contiguous(mem_disp), _lib.contiguous(mem_cost)
        k = mem_disp.shape[1]
        if tuple(mem_disp.shape) != (B, k, h, w) or mem_cost.shape != mem_disp.shape:
            raise RuntimeError("reproject_memory: memory shapes %s / %s, expected [%d,k,%d,%d]"
                               % (tuple(mem_disp.shape), tuple(mem_cost.shape), B, h, w))
    n_in = 0
    if local_map is not None:
        local_map = _lib.contiguous(local_map)
        n_in = local_map.shape[1]
        if tuple(local_map.shape) != (B, n_in, h, w):
            raise RuntimeError("reproject_memory: local map %s, expected [%d,n,%d,%d]" % (tuple(local_map.shape), B, h, w))
    n_local_out = min(int(n_local_out), n_in + 1)
    K, T_a = _lib.contiguous(K), _lib.contiguous(T_a)
    T_b = None if T_b is None else _lib.contiguous(T_b)
    base_t, base_s = None, 0.0
    if torch.is_tensor(baseline):
        if baseline.numel() == 1 and baseline.device.type == 'cpu':
            base_s = float(baseline)
        else:
            base_t = _lib.contiguous(baseline.to(device=dev, dtype=torch.float32).reshape(-1).expand(B))
    else:
        base_s = float(baseline)
    f32 = dict(device=dev, dtype=torch.float32)
    out_d = torch.empty((B, k, h, w), **f32) if k else None
    out_c = torch.empty((B, k, h, w), **f32) if k else None
    out_l = torch.empty((B, n_local_out, h, w), **f32) if n_local_out else None
    L = _lib.lib()
    ws = torch.empty(L.ts_reproject_memory_workspace_bytes(B, h, w, k, n_local_out), device=dev, dtype=torch.uint8)
    opt = lambda t: None if t is None else _lib.ptr(t)
    _lib.check(L.ts_reproject_memory_fwd(_lib.ptr(prev_disp), prev_disp.stride(0), Hf, Wf, opt(mem_disp), opt(mem_cost), k,
                                         opt(local_map), n_in, n_local_out, _lib.ptr(K), K.shape[-1], _lib.ptr(T_a), opt(T_b),
                                         opt(base_t), base_s, float(factor), opt(out_d), opt(out_c), opt(out_l),
                                         _lib.ptr(ws), B, h, w, _stream()), "ts_reproject_memory_fwd")
    return out_d, out_c, out_l


def project_to_3d(depth, K, inv_K=None, T_target_to_source=None, eps=1e-7):
    """project_to_3d of the reference (layers/inverse_warp.py:92-178), forward only (the project
    calls it on detached tensors).  Returns triangular_depth / optical_flow / flow_mask;
    homo_points_3d and src_pixel_coord (= optical_flow + the pixel grid) are not produced: no caller
    on the hot path reads them."""
    if T_target_to_source is None:
        raise NotImplementedError("the hot path always passes T_target_to_source")
    _require_gpu(depth, K, T_target_to_source)
    if inv_K is None:
        inv_K = torch.inverse(K[:, :3, :3])
    depth = _lib.contiguous(depth)
    K, inv_K, T = _lib.contiguous(K), _lib.contiguous(inv_K), _lib.contiguous(T_target_to_source)
    B, C, H, W = depth.shape
    tri = torch.empty_like(depth)
    flow = torch.empty((B, 2 * C, H, W), device=depth.device, dtype=torch.float32)
    mask = torch.empty((B, C, H, W), device=depth.device, dtype=torch.uint8)
    _lib.check(_lib.lib().ts_project_to_3d_fwd(_lib.ptr(depth), _lib.ptr(K), _lib.ptr(inv_K), _lib.ptr(T), _lib.ptr(tri),
                                               _lib.ptr(flow), _lib.ptr(mask), B, C, H, W, K.shape[-1], inv_K.shape[-1],
                                               float(eps), _stream()), "ts_project_to_3d_fwd")
    out = {'triangular_depth': tri, 'optical_flow': flow, 'flow_mask': mask.bool()}
    return out


# ----------------------------------------------------------------------------------- the 2-D inverse warp
_WARP_MODES = {'disparity': 0, 'flow': 1, 'depth': 2}
_WARP_INTERP = {'bilinear': 0, 'nearest': 1, 'bicubic': 2}
_WARP_PAD = {'zeros': 0, 'border': 1, 'reflection': 2}


class _InverseWarp(torch.autograd.Function):
    """ts_inverse_warp_fwd / ts_inverse_warp_bwd.  Returns (warped, triangular_depth, src_pixel_coord, optical_flow, flow_mask,
    homo_points_3d); the last five are None unless `side`, and are marked non-differentiable."""

    @staticmethod
    def forward(ctx, img, motion, K, inv_K, T, codes, eps, side):
        mode, interp, pad = codes
        B, C, Hi, Wi = img.shape
        H, W = motion.shape[2:]
        f32 = dict(device=img.device, dtype=torch.float32)
        out = torch.empty((B, C, H, W), **f32)
        tri = coord = flow = mask = homo = None
        if side:
            tri, coord, flow = torch.empty((B, 1, H, W), **f32), torch.empty((B, 2, H, W), **f32), torch.empty((B, 2, H, W), **f32)
            mask, homo = torch.empty((B, 1, H, W), device=img.device, dtype=torch.uint8), torch.empty((B, 4, H * W), **f32)
        kd = K.shape[-1] if K is not None else 0
        ikd = inv_K.shape[-1] if inv_K is not None else 0
        p = _lib.ptr
        rc = _lib.lib().ts_inverse_warp_fwd(p(img), p(motion), p(K), p(inv_K), p(T), p(out), p(tri), p(coord), p(flow), p(mask), p(homo),
                                            B, C, Hi, Wi, H, W, mode, interp, pad, kd, ikd, float(eps), _stream())
        _lib.check(rc, "ts_inverse_warp_fwd")
        ctx.save_for_backward(img, motion, K, inv_K, T)
        ctx.geom = (codes, kd, ikd, float(eps))
        if side:
            mask = mask.bool()
            ctx.mark_non_differentiable(tri, coord, flow, mask, homo)
        return out, tri, coord, flow, mask, homo

    @staticmethod
    def backward(ctx, g, *_side):
        img, motion, K, inv_K, T = ctx.saved_tensors
        (mode, interp, pad), kd, ikd, eps = ctx.geom
        B, C, Hi, Wi = img.shape
        H, W = motion.shape[2:]
        need_img, need_motion = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_img or need_motion):
            return (None,) * 8
        g = _lib.contiguous(g)
        gi = torch.zeros_like(img) if need_img else None            # accumulated into with atomics: order not deterministic
        gm = torch.empty_like(motion) if need_motion else None      # overwritten: deterministic
        p = _lib.ptr
        rc = _lib.lib().ts_inverse_warp_bwd(p(img), p(motion), p(K), p(inv_K), p(T), p(g), p(gi), p(gm), B, C, Hi, Wi, H, W,
                                            mode, interp, pad, kd, ikd, eps, _stream())
        _lib.check(rc, "ts_inverse_warp_bwd")
        return (gi, gm) + (None,) * 6


def mesh_grid(b, h, w, device, dtype=torch.float):
    """mesh_grid of the reference (layers/inverse_warp.py:80-90): pixel coordinates [b, 2, h, w], x then y."""
    x_range = torch.arange(0, w, device=device, dtype=dtype).view(1, 1, 1, w).expand(b, 1, h, w)
    y_range = torch.arange(0, h, device=device, dtype=dtype).view(1, 1, h, 1).expand(b, 1, h, w)
    return torch.cat((x_range, y_range), dim=1)


def inverse_warp(img, motion, mode='disparity', K=None, inv_K=None, T_target_to_source=None, interpolate_mode='bilinear',
                 padding_mode='zeros', eps=1e-7, output_all=False):
    """inverse_warp of the reference (layers/inverse_warp.py:6-77; same arguments, order and defaults): img [B,C,Hi,Wi] sampled at
    the source position of every pixel of motion -- [B,1,H,W] disparity (X = x + m) or depth (X, Y = src_pixel_coord of
    project_to_3d with K, inv_K, T_target_to_source), [B,2,H,W] flow -- through the reference's normalise / grid_sample
    (align_corners=True) round trip, in one launch.  interpolate_mode 'bilinear' | 'nearest' ('bicubic' is refused by the library);
    padding_mode 'zeros' | 'border' | 'reflection'.  Differentiable in img (atomics: summation order not deterministic) and motion
    (deterministic); K, inv_K and T_target_to_source are constants and are refused if they require grad.

    output_all=True returns (projected_img, output): in depth mode the reference's five keys (homo_points_3d, triangular_depth,
    flow_mask (bool), src_pixel_coord, optical_flow) from the same launch, else {}.  The one difference to the reference: these side
    outputs are not differentiable.  inv_K=None means torch.inverse(K[:, :3, :3]).  Depth mode without T_target_to_source raises a
    ValueError (the reference fails there with a bare KeyError)."""
    if img.dim() != 4 or motion.dim() != 4:
        raise ValueError("inverse_warp: img must be [B,C,Hi,Wi] and motion [B,1|2,H,W], got %s and %s" % (tuple(img.shape), tuple(motion.shape)))
    B, C, H, W = motion.shape
    if mode == 'disparity':
        assert C == 1, "Disparity map must be 1 channel, but {} got!".format(C)
    elif mode == 'flow':
        assert C == 2, "Optical flow map must be 2 channel, but {} got!".format(C)
    elif mode == 'depth':
        assert C == 1, "Disparity map must be 1 channel, but {} got!".format(C)
    else:
        raise TypeError("Inverse warp only support [disparity, flow, depth] mode, but {} got".format(mode))
    if interpolate_mode not in _WARP_INTERP:
        raise ValueError("inverse_warp: unknown interpolate_mode %r" % (interpolate_mode,))
    if padding_mode not in _WARP_PAD:
        raise ValueError("inverse_warp: unknown padding_mode %r" % (padding_mode,))
    if img.shape[0] != B:
        raise ValueError("inverse_warp: img and motion differ in batch size (%d and %d)" % (img.shape[0], B))
    depth = mode == 'depth'
    if depth:
        if K is None:
            raise ValueError("inverse_warp: mode='depth' needs the intrinsics K")
        if T_target_to_source is None:
            raise ValueError("inverse_warp: mode='depth' needs T_target_to_source: without it project_to_3d yields no "
                             "src_pixel_coord to sample at")
        for name, t in (("K", K), ("inv_K", inv_K), ("T_target_to_source", T_target_to_source)):
            if t is not None and t.requires_grad:
                raise RuntimeError("inverse_warp: %s requires grad, but it is a constant of the HIP kernel (no gradient reaches it)" % name)
        # the kernel indexes K, inv_K and T by the motion's batch element: a batch of 1 does not broadcast here, it is refused
        for name, t, dims in (("K", K, (3, 4)), ("inv_K", inv_K, (3, 4)), ("T_target_to_source", T_target_to_source, (4,))):
            if t is not None and (t.dim() != 3 or t.shape[0] != B or t.shape[1] != t.shape[2] or t.shape[1] not in dims):
                raise ValueError("inverse_warp: %s must be [%d, k, k] with k in %s (the motion's batch size), got %s"
                                 % (name, B, dims, tuple(t.shape)))
        _require_gpu(img, motion, K, inv_K, T_target_to_source)
        if inv_K is None:
            inv_K = torch.inverse(K[:, :3, :3])
        K, inv_K, T = _lib.contiguous(K), _lib.contiguous(inv_K), _lib.contiguous(T_target_to_source)
    else:
        _require_gpu(img, motion)
        K = inv_K = T = None
    codes = (_WARP_MODES[mode], _WARP_INTERP[interpolate_mode], _WARP_PAD[padding_mode])
    res = _InverseWarp.apply(_lib.contiguous(img), _lib.contiguous(motion), K, inv_K, T, codes, eps, bool(output_all and depth))
    if not output_all:
        return res[0]
    output = {}
    if depth:
        output = {'homo_points_3d': res[5], 'triangular_depth': res[1], 'flow_mask': res[4], 'src_pixel_coord': res[2],
                  'optical_flow': res[3]}
    return res[0], output


# ------------------------------------------- CorrBlock and FlowCorrBlock: the correlation pyramids of RAFT-Stereo (1-D) and RAFT (2-D)
class _CorrKind:
    """What differs on the host between the two correlation pyramids: CorrBlock's row correlation for disparity
    (csrc/raft_corr.hip) and FlowCorrBlock's all-pairs cost for flow (csrc/flow_corr.hip).  Their C entries
    ts_<prefix>_{pyramid,lookup}_{fwd,bwd} have the same signatures and conventions (include/ts_hip.h), so the buffer layout,
    the level count of a buffer, the argument checks and the autograd Functions below are written once over a kind."""

    def __init__(self, prefix, max_levels, motion, channels, level_shapes, level_ok, window_dims, map_name, refuse_levels):
        self.prefix = prefix                    # of the C entries and of every message
        self.max_levels = max_levels            # what one launch of the kind's build kernel pools
        self.motion, self.channels = motion, channels       # the lookup's argument: its name and its channel count
        self.level_shapes = level_shapes        # (H, W, num_levels) -> [(h_i, w_i)], the target map of every level
        self.level_ok = level_ok                # (h_i, w_i) -> whether such a level exists
        self.window_dims = window_dims          # a level's window has (2 * radius + 1) ** window_dims taps
        self.map_name = map_name                # (H, W) -> what a message calls the target map
        self.refuse_levels = refuse_levels      # (H, W, num_levels): raises the kind's own refusal of a map or a level
        # The entries' names.  A caller resolves them on _lib.lib() when it calls, never sooner: a plan Recorder swaps its proxy
        # in per thread.  (Spelled out at the call sites: the lookups are launch-bound and a helper's frame shows in their time.)
        self.pyramid_fwd, self.pyramid_bwd, self.lookup_fwd, self.lookup_bwd = (
            "ts_%s_%s" % (prefix, e) for e in ("pyramid_fwd", "pyramid_bwd", "lookup_fwd", "lookup_bwd"))

    def level_views(self, pyramid, B, H, W, num_levels):
        N, views, o = B * H * W, [], 0
        for h, w in self.level_shapes(H, W, num_levels):
            n = N * h * w
            views.append(pyramid[o:o + n].view(N, 1, h, w))
            o += n
        return views

    def levels_of(self, pyramid, N, H, W):
        """num_levels of a pyramid buffer of N source pixels over an H x W map: its length decides (a level that does not exist
        adds nothing to the length and is not counted)."""
        if pyramid.dim() != 1 or N <= 0 or pyramid.numel() % N:
            raise ValueError("%s_lookup: pyramid must be the 1-D buffer of %s_pyramid for %d pixels, got %s"
                             % (self.prefix, self.prefix, N, tuple(pyramid.shape)))
        per, s = pyramid.numel() // N, 0
        for i, (h, w) in enumerate(self.level_shapes(H, W, self.max_levels)):
            s += h * w
            if s == per and self.level_ok(h, w):
                return i + 1
        raise ValueError("%s_lookup: a pyramid of %d floats per pixel is no pyramid of %s" % (self.prefix, per, self.map_name(H, W)))

    def check_features(self, fmap1, fmap2, num_levels):
        s1, s2 = tuple(fmap1.shape), tuple(fmap2.shape)
        if len(s1) != 4 or len(s2) != 4:
            raise ValueError("%s: fmap1 and fmap2 must be [B,C,H,W], got %s and %s" % (self.prefix, s1, s2))
        if s1 != s2:
            raise ValueError("%s: fmap1 and fmap2 differ in shape (%s and %s)" % (self.prefix, s1, s2))
        if num_levels < 1:
            raise ValueError("%s: num_levels must be >= 1, got %d" % (self.prefix, num_levels))
        if num_levels > self.max_levels:
            raise ValueError("%s: num_levels = %d, the HIP kernel pools at most %d levels" % (self.prefix, num_levels, self.max_levels))
        self.refuse_levels(s1[2], s1[3], num_levels)
        _require_gpu(fmap1, fmap2)

    def check_motion(self, motion, radius, size=None):
        shape = tuple(motion.shape)         # once: every `.shape` builds a new object, and the lookups are launch-bound
        if len(shape) != 4 or shape[1] != self.channels:
            raise ValueError("%s: %s must be [B,%d,H,W] (%d channel%s), got %s"
                             % (self.prefix, self.motion, self.channels, self.channels, "s" * (self.channels > 1), shape))
        if size is not None and (shape[0], shape[2], shape[3]) != size:
            raise ValueError("%s: %s %s does not match the feature maps' (B, H, W) = %s" % (self.prefix, self.motion, shape, size))
        if radius < 0:
            raise ValueError("%s: radius must be >= 0, got %d" % (self.prefix, radius))


def _raft_refuse_levels(H, W, num_levels):
    if W < 2:
        raise ValueError("raft_corr: W = %d, need W >= 2 (the lookup divides by W - 1)" % W)
    if (W >> (num_levels - 1)) < 1:
        raise ValueError("raft_corr: W = %d is too narrow for num_levels = %d (level %d would be empty; the reference's "
                         "avg_pool2d raises there)" % (W, num_levels, num_levels - 1))


def _flow_refuse_levels(H, W, num_levels):
    for i in range(num_levels):
        if (H >> i) < 2 or (W >> i) < 2:
            raise ValueError("flow_corr: level %d of a %d x %d map is %d x %d, need >= 2 x 2 (the lookup divides by H_i - 1 and "
                             "W_i - 1)" % (i, H, W, H >> i, W >> i))


# The level limits: 7 is kMaxLevels of csrc/corr_common.hpp, the deepest level the 64-wide tile of csrc/raft_corr.hip still pools by
# itself (64 >> 6 == 1); csrc/flow_corr.hip pools levels 1..3 from an 8-row patch of the level-0 tile, hence 4.
_RAFT = _CorrKind("raft_corr", 7, "disp", 1, lambda H, W, L: [(1, W >> i) for i in range(L)], lambda h, w: w >= 1, 1,
                  lambda H, W: "width %d" % W, _raft_refuse_levels)
_FLOW = _CorrKind("flow_corr", 4, "coords", 2, lambda H, W, L: [(H >> i, W >> i) for i in range(L)], lambda h, w: h >= 2 and w >= 2, 2,
                  lambda H, W: "a %d x %d map" % (H, W), _flow_refuse_levels)


class _CorrPyramid(torch.autograd.Function):
    """ts_*_corr_pyramid_fwd / ts_*_corr_pyramid_bwd (the cotangent keeps its levels: folded while it is staged)."""

    @staticmethod
    def forward(ctx, kind, fmap1, fmap2, num_levels):
        B, C, H, W = fmap1.shape
        pyr = torch.empty(B * H * W * sum([h * w for h, w in kind.level_shapes(H, W, num_levels)]), device=fmap1.device, dtype=torch.float32)
        p, entry = _lib.ptr, kind.pyramid_fwd
        _lib.check(getattr(_lib.lib(), entry)(p(fmap1), p(fmap2), p(pyr), B, C, H, W, num_levels, _stream()), entry)
        ctx.save_for_backward(fmap1, fmap2)
        ctx.geom = (kind, num_levels)
        return pyr

    @staticmethod
    def backward(ctx, g):
        fmap1, fmap2 = ctx.saved_tensors
        kind, L = ctx.geom
        B, C, H, W = fmap1.shape
        g1 = torch.empty_like(fmap1) if ctx.needs_input_grad[1] else None
        g2 = torch.empty_like(fmap2) if ctx.needs_input_grad[2] else None
        if g1 is None and g2 is None:
            return None, None, None, None
        g = _lib.contiguous(g)
        p = _lib.ptr
        _lib.check(getattr(_lib.lib(), kind.pyramid_bwd)(p(g), p(fmap1), p(fmap2), p(g1), p(g2), B, C, H, W, L, _stream()), kind.pyramid_bwd)
        return None, g1, g2, None


def _corr_lookup_fwd(kind, pyramid, motion, num_levels, radius):
    B, _, H, W = motion.shape
    out = torch.empty((B, num_levels * (2 * radius + 1) ** kind.window_dims, H, W), device=motion.device, dtype=torch.float32)
    p, entry = _lib.ptr, kind.lookup_fwd
    _lib.check(getattr(_lib.lib(), entry)(p(pyramid), p(motion), p(out), B, H, W, num_levels, radius, _stream()), entry)
    return out


class _CorrLookup(torch.autograd.Function):
    """ts_*_corr_lookup_fwd / ts_*_corr_lookup_bwd with fold = 0: the gradient with respect to a free pyramid, level by level."""

    @staticmethod
    def forward(ctx, kind, pyramid, motion, num_levels, radius):
        ctx.save_for_backward(pyramid, motion)
        ctx.geom = (kind, num_levels, radius)
        return _corr_lookup_fwd(kind, pyramid, motion, num_levels, radius)

    @staticmethod
    def backward(ctx, g):
        pyramid, motion = ctx.saved_tensors
        kind, L, r = ctx.geom
        B, _, H, W = motion.shape
        gp = torch.empty_like(pyramid) if ctx.needs_input_grad[1] else None
        gm = torch.empty_like(motion) if ctx.needs_input_grad[2] else None
        if gp is None and gm is None:
            return None, None, None, None, None
        g = _lib.contiguous(g)
        p = _lib.ptr
        _lib.check(getattr(_lib.lib(), kind.lookup_bwd)(p(pyramid), p(motion), p(g), p(gm), p(gp), B, H, W, L, r, 0, _stream()), kind.lookup_bwd)
        return None, gp, gm, None, None


class _CorrBlockLookup(torch.autograd.Function):
    """The lookup of a block, differentiable in the FEATURES the pyramid was built from: backward is ts_*_corr_lookup_bwd with
    fold = 1 (one [B*H*W, h_0*w_0] cotangent of level 0, written once) and ts_*_corr_pyramid_bwd on it with levels = 1 -- the
    per-level cotangent of the pyramid is never materialised."""

    @staticmethod
    def forward(ctx, kind, fmap1, fmap2, pyramid, motion, num_levels, radius):
        ctx.save_for_backward(fmap1, fmap2, pyramid, motion)
        ctx.geom = (kind, num_levels, radius)
        return _corr_lookup_fwd(kind, pyramid, motion, num_levels, radius)

    @staticmethod
    def backward(ctx, g):
        fmap1, fmap2, pyramid, motion = ctx.saved_tensors
        kind, L, r = ctx.geom
        B, C, H, W = fmap1.shape
        _, need1, need2, _, needm = ctx.needs_input_grad[:5]
        if not (need1 or need2 or needm):
            return (None,) * 7
        g = _lib.contiguous(g)
        p = _lib.ptr
        feats = need1 or need2
        (h0, w0), = kind.level_shapes(H, W, 1)
        G = torch.empty(B * H * W * h0 * w0, device=g.device, dtype=torch.float32) if feats else None
        gm = torch.empty_like(motion) if needm else None
        _lib.check(getattr(_lib.lib(), kind.lookup_bwd)(p(pyramid), p(motion), p(g), p(gm), p(G), B, H, W, L, r, 1, _stream()), kind.lookup_bwd)
        g1 = torch.empty_like(fmap1) if need1 else None
        g2 = torch.empty_like(fmap2) if need2 else None
        if feats:
            _lib.check(getattr(_lib.lib(), kind.pyramid_bwd)(p(G), p(fmap1), p(fmap2), p(g1), p(g2), B, C, H, W, 1, _stream()), kind.pyramid_bwd)
        return None, g1, g2, None, gm, None, None


def _corr_pyramid(kind, fmap1, fmap2, num_levels):
    num_levels = int(num_levels)
    kind.check_features(fmap1, fmap2, num_levels)
    return _CorrPyramid.apply(kind, _lib.contiguous(fmap1), _lib.contiguous(fmap2), num_levels)


def _corr_lookup(kind, pyramid, motion, radius, size=None):
    """Refusals in one order for both kinds: the arguments' shapes and values, the buffer's length, then device and dtype."""
    radius = int(radius)
    kind.check_motion(motion, radius)
    B, _, H, W = motion.shape
    if size is not None and tuple(size) != (H, W):
        raise ValueError("%s: %s %s does not match size = %s" % (kind.prefix, kind.motion, tuple(motion.shape), tuple(size)))
    kind.refuse_levels(H, W, 1)
    L = kind.levels_of(pyramid, B * H * W, H, W)
    _require_gpu(pyramid, motion)
    return _CorrLookup.apply(kind, _lib.contiguous(pyramid), _lib.contiguous(motion), L, radius)


def raft_corr_pyramid(fmap1, fmap2, num_levels):
    """The correlation pyramid of the reference's CorrBlock (aggregation/utils/raft_corr.py:15-22, :55-67) in one launch:
    level 0 is the all-pairs row correlation sum_c fmap1[b,c,y,x] fmap2[b,c,y,x'] / sqrt(C), level i the average of adjacent
    pairs of level i-1 along x' (an odd tail is dropped).  Returns ONE 1-D fp32 buffer: level i is [B*H*W, W >> i] contiguous
    at offset B*H*W * (W + (W >> 1) + ... + (W >> (i-1))) -- `raft_corr_level_views` slices it.  Differentiable in both maps."""
    return _corr_pyramid(_RAFT, fmap1, fmap2, num_levels)


def raft_corr_lookup(pyramid, disp, radius):
    """The windowed lookup of the reference's CorrBlock.__call__ (raft_corr.py:24-53) in one launch: out [B, L*(2r+1), H, W],
    channel i*(2r+1)+k = (1 - 2^-(i+1)) * the linear interpolation (zeros outside) of level i's row of the pixel at
    ((x - disp) / 2^i + (k - r)) * (W >> i) / (W - 1) - 0.5.  `pyramid` is the buffer of raft_corr_pyramid for the same B, H, W
    (the number of levels follows from its length).  Differentiable in the pyramid (every level) and in disp."""
    return _corr_lookup(_RAFT, pyramid, disp, radius)


def raft_corr_level_views(pyramid, B, H, W, num_levels):
    """The levels of a pyramid buffer as the reference's `corr_pyramid` entries: [B*H*W, 1, 1, W >> i] views (no copies)."""
    return _RAFT.level_views(pyramid, B, H, W, num_levels)


def flow_corr_pyramid(fmap1, fmap2, num_levels):
    """The correlation pyramid of the reference's FlowCorrBlock (aggregation/utils/raft_corr.py:73-87, :112-123) in one launch:
    level 0 is the all-pairs cost (f1_n.f1_m - 2 f1_n.f2_m + f2_n.f2_m) / sqrt(C) between pixel n of fmap1 and pixel m of fmap2
    (the reference's full Gram matrices), level i the 2x2 average of level i-1 over m (an odd last row or column is dropped).
    Returns ONE 1-D fp32 buffer: level i is [B*H*W, (H >> i)*(W >> i)] contiguous, stored after the levels before it --
    `flow_corr_level_views` slices it.  Differentiable in both maps."""
    return _corr_pyramid(_FLOW, fmap1, fmap2, num_levels)


def flow_corr_lookup(pyramid, coords, radius, size=None):
    """The windowed lookup of the reference's FlowCorrBlock.__call__ (raft_corr.py:89-110, bilinear_sampler :146-160) in one launch:
    out [B, L*(2r+1)^2, H, W], channel i*(2r+1)^2 + a*(2r+1) + b = the bilinear sample (zeros outside) of pixel (y, x)'s level-i
    row at (coords_x / 2^i + a - r, coords_y / 2^i + b - r): the first window index moves x, as the reference's does.  `pyramid`
    is the buffer of flow_corr_pyramid for the same B, H, W (`size` = (H, W), by default coords' own; the number of levels
    follows from the buffer's length).  Differentiable in the pyramid (every level) and in coords."""
    return _corr_lookup(_FLOW, pyramid, coords, radius, size)


def flow_corr_level_views(pyramid, B, H, W, num_levels):
    """The levels of a pyramid buffer as the reference's `corr_pyramid` entries: [B*H*W, 1, H >> i, W >> i] views (no copies)."""
    return _FLOW.level_views(pyramid, B, H, W, num_levels)


class _CorrBlockBase:
    """What CorrBlock and FlowCorrBlock share: the pyramid is built in one launch into one buffer, of which `corr_pyramid[i]` is
    the view of level i, and a call looks the window up on every level in one launch.

    Gradients reach the call's argument and the two feature maps through the call (the pyramid's per-level cotangent is never
    materialised: ts_*_corr_lookup_bwd folds it into one level-0 cotangent, ts_*_corr_pyramid_bwd contracts that); the
    `corr_pyramid` views themselves carry no gradient.  No host reads: build and lookup can be captured."""

    _kind = None

    def __init__(self, fmap1, fmap2, num_levels=4, radius=4):
        kind = self._kind
        num_levels, radius = int(num_levels), int(radius)
        if radius < 0:
            raise ValueError("%s: radius must be >= 0, got %d" % (kind.prefix, radius))
        kind.check_features(fmap1, fmap2, num_levels)
        self.num_levels = num_levels
        self.radius = radius
        f1, f2 = _lib.contiguous(fmap1), _lib.contiguous(fmap2)
        with torch.no_grad():
            self._pyramid = _CorrPyramid.apply(kind, f1, f2, num_levels)
        self._shape = tuple(fmap1.shape)
        # the feature maps are kept only where a backward can ask for them (the reference keeps the pyramid alone)
        self._fmaps = (f1, f2) if torch.is_grad_enabled() and (f1.requires_grad or f2.requires_grad) else None
        B, _, H, W = self._shape
        self.corr_pyramid = kind.level_views(self._pyramid, B, H, W, num_levels)

    def __call__(self, motion):
        kind = self._kind
        B, _, H, W = self._shape
        kind.check_motion(motion, self.radius, (B, H, W))
        _require_gpu(motion)
        motion = _lib.contiguous(motion)
        if self._fmaps is None:
            return _CorrLookup.apply(kind, self._pyramid, motion, self.num_levels, self.radius)
        return _CorrBlockLookup.apply(kind, self._fmaps[0], self._fmaps[1], self._pyramid, motion, self.num_levels, self.radius)


class CorrBlock(_CorrBlockBase):
    """CorrBlock of the reference (aggregation/utils/raft_corr.py:4-67; same arguments and attributes), for disparity: the
    all-pairs row correlation of fmap1 and fmap2 [B,C,H,W] as a pyramid of `num_levels` levels, and `__call__(disp)` with
    disp [B,1,H,W]: the (2*radius+1)-tap bilinear window around x - disp on every level, [B, num_levels*(2*radius+1), H, W].
    `corr_pyramid[i]` is the [B*H*W, 1, 1, W >> i] view of level i."""

    _kind = _RAFT


class FlowCorrBlock(_CorrBlockBase):
    """FlowCorrBlock of the reference (aggregation/utils/raft_corr.py:71-144; same arguments and attributes), for optical flow:
    the all-pairs cost between every pixel of fmap1 and every pixel of fmap2 [B,C,H,W] as a pyramid of `num_levels` levels, and
    `__call__(coords)` with coords [B,2,H,W] (x, y): the (2*radius+1)^2 bilinear window around the target coordinate on every
    level, [B, num_levels*(2*radius+1)^2, H, W].  `corr_pyramid[i]` is the [B*H*W, 1, H >> i, W >> i] view of level i."""

    _kind = _FLOW

    @staticmethod
    def init_flow(size, device, flow_init=None):
        """(ref_coord, tgt_coord) of raft_corr.py:125-144: the pixel grid [B,2,H,W] (channel 0 = x, 1 = y) of a [B,C,H,W] `size`,
        the target moved by `flow_init` when given.  Plain torch."""
        if len(size) != 4:
            raise ValueError("flow_corr: init_flow expects a size [B, C, H, W], got %s" % (tuple(size),))
        b, _, h, w = size
        xs = torch.arange(0, w, device=device, dtype=torch.float).view(1, 1, 1, w).expand(b, 1, h, w)
        ys = torch.arange(0, h, device=device, dtype=torch.float).view(1, 1, h, 1).expand(b, 1, h, w)
        grid = torch.cat((xs, ys), dim=1).detach()
        return grid, (grid if flow_init is None else grid + flow_init)


# ---- ConvGRU (reference: layers/conv_gru.py:4-28) --------------------------------------------------------------------------------------
CONV_GRU_MAX_PLANES = 64          # the kernel path's envelope on either side (csrc/conv_gru.hip)


def conv_gru_supported(hidden_planes, in_planes):
    return 1 <= hidden_planes <= CONV_GRU_MAX_PLANES and 1 <= in_planes <= CONV_GRU_MAX_PLANES


def _dense_planes(t):
    """Whether the kernels can read or write a [B,C,H,W] tensor in place: dense planes, batch / channel strides that do not overlap."""
    B, C, H, W = t.shape
    return t.stride(3) == 1 and t.stride(2) == W and t.stride(1) >= H * W and (B == 1 or t.stride(0) >= t.stride(1) * (C - 1) + H * W)


def _plane_view(t):
    """A [B,C,H,W] tensor the kernels can read in place (`_dense_planes`), else a copy."""
    return t if _dense_planes(t) else _lib.contiguous(t)


def _optional_operand(t):
    """(tensor, batch stride, channel stride) of an optional strided operand (a residual, the memory) as an entry takes it: read in
    place where `_plane_view` allows; (None, 0, 0) when absent."""
    if t is None:
        return None, 0, 0
    t = _plane_view(t)
    return t, t.stride(0), t.stride(1)


def _node_weight_layout(tag, entry, refusal, *extra):
    """-> lay(weight): the kernel image of a [Cout, Cin, ...] weight of one 2-D node family, through `entry`_bytes(Cin, Cout, *extra) and
    `entry`_layout(w, w_l, Cin, Cout, *extra, stream) (one launch).  Inside a `WeightLayouts` context a leaf is laid out once per step
    and refreshed with the others under `tag`; the maker is built here, once, so that context can keep and call it.  A weight outside
    the entry's envelope raises RuntimeError(refusal % (Cin, Cout, *extra))."""
    def make(weight, out=None):
        Cout, Cin = weight.shape[0], weight.shape[1]
        if out is None:
            nbytes = _q(entry + "_bytes", Cin, Cout, *extra)
            if not nbytes:
                raise RuntimeError(refusal % ((Cin, Cout) + extra))
            out = torch.empty(nbytes // 4, device=weight.device, dtype=torch.float32)
        _lib.check(getattr(_lib.lib(), entry + "_layout")(_lib.ptr(weight.detach()), _lib.ptr(out), Cin, Cout, *extra, _stream()), entry + "_layout")
        return out

    def lay(weight):
        if _LAYOUTS is not None and weight.is_contiguous() and weight.is_leaf:
            return _LAYOUTS.get_custom(weight, tag, make)
        return make(_lib.contiguous(weight.detach()))
    return lay


def _fold_check(what, name, fold, n, required=False):
    """-> (scale, shift) of a BatchNorm fold of at least n channels, (None, None) for no fold"""
    if fold is None and not required:
        return None, None
    if fold is None or len(fold) != 2 or any(v is None or v.dim() != 1 or v.numel() < n or not v.is_contiguous() for v in fold):
        raise ValueError("%s: the %s fold must be a (scale, shift) pair of dense vectors of at least %d values" % (what, name, n))
    return fold


def _out_check(what, name, t, shape):
    """A [B,C,H,W] operand the kernels write (or read as the residual) in place: `_dense_planes` of exactly `shape`."""
    if tuple(t.shape) != tuple(shape) or not _dense_planes(t):
        raise ValueError("%s: %s must be %s with dense planes and strides that do not overlap, got %s strides %s"
                         % (what, name, list(shape), tuple(t.shape), tuple(t.stride())))


def _gru_bwd_weight_layout(ws, Cin):
    """[sum of rows][9][pad(Cin)] with the taps flipped: the array ts_conv3d_hw_bwd_data takes for the convolution whose output rows are
    the rows of `ws` stacked (one ts_conv_weight_layout launch per weight, into its slice)."""
    cp = _cpad(Cin)
    rows = sum(w.shape[0] for w in ws)
    out = torch.empty((rows, 9, cp), device=ws[0].device, dtype=torch.float32)
    at = 0
    for w in ws:
        n = w.shape[0]
        _lib.check(_lib.lib().ts_conv_weight_layout(_lib.ptr(w), _lib.ptr(out[at:]), n, 9, Cin, cp, Cin * 9, 9, 1, 1, _stream()),
                   "ts_conv_weight_layout")
        at += n
    return out


_WGRAD_MAX_COUT = 64              # ts_conv3d_hw_bwd_weight holds at most 64 output channels


def _wgrad_by_source(sources, dy):
    """dw [Cout, sum of channels, 3, 3] of a 3x3 convolution whose input channels come from several tensors: `sources` is the list of
    (source [B,c,H,W], c) in channel order, dy a [B,Cout,H,W] view with a dense plane.  ts_conv3d_hw_bwd_weight holds at most 64 output
    channels and reads one source, so it runs per slice of dy's channels and per source; the blocks are joined along the input channels,
    then along the rows."""
    L, st = _lib.lib(), _stream()
    B, Cout, H, W = dy.shape
    rows = []
    for co in range(0, Cout, _WGRAD_MAX_COUT):
        n = min(_WGRAD_MAX_COUT, Cout - co)
        dy_s = dy[:, co:co + n]
        parts = []
        for src, cin in sources:
            part = torch.empty((n, cin, 3, 3), device=dy.device, dtype=torch.float32)
            ws, nws = _wgrad_workspace(cin, n, 9, dy.device)
            rc = L.ts_conv3d_hw_bwd_weight(_lib.ptr(src), _lib.ptr(dy_s), _lib.ptr(part), B, cin, n, 1, H, W, 1, 1, src.stride(0),
                                           src.stride(1), dy.stride(0), dy.stride(1), _lib.ptr(ws), nws, st)
            _lib.check(rc, "ts_conv3d_hw_bwd_weight")
            parts.append(part)
        rows.append(parts[0] if len(parts) == 1 else torch.cat(parts, 1))
    return rows[0] if len(rows) == 1 else torch.cat(rows, 0)


class _ConvGRU(torch.autograd.Function):
    """hidden = (1 - z) * h + z * q of the gated recurrent cell in two launches (ts_conv_gru_gates_fwd, ts_conv_gru_out_fwd) after
    one weight-layout launch; h and x are read in place.  r and q are kept only when a backward pass can ask for them.
    backward: ts_conv_gru_gate_bwd_a -> candidate convolution's gradients -> ts_conv_gru_gate_bwd_b -> gate convolutions' gradients ->
    ts_conv_gru_grad_sum; the convolutions' own gradients on ts_conv3d_hw_bwd_{data,weight} (D = 1), the biases' on ts_channel_sum_fwd."""

    @staticmethod
    def forward(ctx, h, x, wz, bz, wr, br, wq, bq, gates):
        _require_gpu(h, x, wz, bz, wr, br, wq, bq)
        if h.dim() != 4 or x.dim() != 4 or h.shape[0] != x.shape[0] or h.shape[2:] != x.shape[2:]:
            raise ValueError("conv_gru: last_hidden [B,Ch,H,W] and x [B,Cx,H,W] expected, got %s and %s" % (tuple(h.shape), tuple(x.shape)))
        B, Ch, H, W = h.shape
        Cx = x.shape[1]
        for w in (wz, wr, wq):
            if tuple(w.shape) != (Ch, Ch + Cx, 3, 3):
                raise ValueError("conv_gru: weights must be [%d, %d, 3, 3], got %s" % (Ch, Ch + Cx, tuple(w.shape)))
        for b in (bz, br, bq):
            if tuple(b.shape) != (Ch,):
                raise ValueError("conv_gru: biases must be [%d], got %s" % (Ch, tuple(b.shape)))
        h, x = _plane_view(h), _plane_view(x)
        wz, wr, wq = (_lib.contiguous(w.detach()) for w in (wz, wr, wq))
        bz, br, bq = (_lib.contiguous(b.detach()) for b in (bz, br, bq))
        train = any(ctx.needs_input_grad[:8])
        L = _lib.lib()
        nbytes = _q("ts_conv_gru_weight_bytes", Ch, Cx)
        if not nbytes:
            raise RuntimeError("conv_gru: %d hidden / %d input planes are outside the kernel path (1..%d each)" % (Ch, Cx, CONV_GRU_MAX_PLANES))
        w_l = torch.empty(nbytes // 4, device=h.device, dtype=torch.float32)
        _lib.check(L.ts_conv_gru_weight_layout(_lib.ptr(wz), _lib.ptr(wr), _lib.ptr(wq), _lib.ptr(w_l), Ch, Cx, _stream()),
                   "ts_conv_gru_weight_layout")
        new = lambda: torch.empty((B, Ch, H, W), device=h.device, dtype=torch.float32)
        keep = train or gates
        z, rh, out = new(), new(), new()
        r, q = (new(), new()) if keep else (None, None)
        strides = (h.stride(0), h.stride(1), x.stride(0), x.stride(1))
        _lib.check(L.ts_conv_gru_gates_fwd(_lib.ptr(h), _lib.ptr(x), _lib.ptr(w_l), _lib.ptr(bz), _lib.ptr(br), _lib.ptr(z), _lib.ptr(rh),
                                           _lib.ptr(r), B, Ch, Cx, H, W, *strides, _stream()), "ts_conv_gru_gates_fwd")
        _lib.check(L.ts_conv_gru_out_fwd(_lib.ptr(rh), _lib.ptr(x), _lib.ptr(w_l), _lib.ptr(bq), _lib.ptr(z), _lib.ptr(h), _lib.ptr(out),
                                         _lib.ptr(q), B, Ch, Cx, H, W, *strides, _stream()), "ts_conv_gru_out_fwd")
        if train:
            ctx.save_for_backward(h, x, wz, wr, wq, z, r, q, rh)
        if gates:
            ctx.mark_non_differentiable(z, r, q)
            return out, z, r, q
        return out

    @staticmethod
    def backward(ctx, dout, *unused):
        h, x, wz, wr, wq, z, r, q, rh = ctx.saved_tensors
        need = ctx.needs_input_grad
        B, Ch, H, W = h.shape
        Cx, C, N = x.shape[1], h.shape[1] + x.shape[1], H * W
        L, st = _lib.lib(), _stream()
        dout = _lib.contiguous(dout)
        dev = h.device
        new = lambda c: torch.empty((B, c, H, W), device=dev, dtype=torch.float32)
        dq_pre, dgate, dh = new(Ch), new(2 * Ch), new(Ch)              # dgate = [dz_pre | dr_pre]: the gate convolution's cotangent
        _lib.check(L.ts_conv_gru_gate_bwd_a(_lib.ptr(dout), _lib.ptr(z), _lib.ptr(q), _lib.ptr(h), _lib.ptr(dq_pre), _lib.ptr(dgate),
                                            _lib.ptr(dh), B, Ch, N, h.stride(0), h.stride(1), 2 * Ch * N, N, st), "ts_conv_gru_gate_bwd_a")
        dcat_q, dcat_g = new(C), new(C)
        rc = L.ts_conv3d_hw_bwd_data(_lib.ptr(dq_pre), _lib.ptr(_gru_bwd_weight_layout((wq,), C)), _lib.ptr(dcat_q), B, C, Ch, 1, H, W, 1, 1, 0,
                                     Ch * N, N, C * N, N, st)
        _lib.check(rc, "ts_conv3d_hw_bwd_data")
        dr_pre = dgate[:, Ch:]
        _lib.check(L.ts_conv_gru_gate_bwd_b(_lib.ptr(dcat_q), _lib.ptr(r), _lib.ptr(h), _lib.ptr(dr_pre), _lib.ptr(dh), B, Ch, N, C * N, N,
                                            h.stride(0), h.stride(1), 2 * Ch * N, N, st), "ts_conv_gru_gate_bwd_b")
        rc = L.ts_conv3d_hw_bwd_data(_lib.ptr(dgate), _lib.ptr(_gru_bwd_weight_layout((wz, wr), C)), _lib.ptr(dcat_g), B, C, 2 * Ch, 1, H, W,
                                     1, 1, 0, 2 * Ch * N, N, C * N, N, st)
        _lib.check(rc, "ts_conv3d_hw_bwd_data")
        dx = new(Cx) if need[1] else None
        _lib.check(L.ts_conv_gru_grad_sum(_lib.ptr(dcat_g), _lib.ptr(dcat_q), _lib.ptr(dh), _lib.ptr(dx), B, Ch, Cx, N, st),
                   "ts_conv_gru_grad_sum")

        dwz = _wgrad_by_source(((h, Ch), (x, Cx)), dgate[:, :Ch]) if need[2] else None          # Ch <= 64: one slice each
        dwr = _wgrad_by_source(((h, Ch), (x, Cx)), dr_pre) if need[4] else None
        dwq = _wgrad_by_source(((rh, Ch), (x, Cx)), dq_pre) if need[6] else None
        dbz = dbr = dbq = None
        if need[3] or need[5]:
            both = _channel_sum(dgate)
            dbz, dbr = (both[:Ch] if need[3] else None), (both[Ch:] if need[5] else None)
        if need[7]:
            dbq = _channel_sum(dq_pre)
        return (dh if need[0] else None), dx, dwz, dbz, dwr, dbr, dwq, dbq, None


def conv_gru(last_hidden, x, wz, bz, wr, br, wq, bq, return_gates=False):
    """One step of the gated recurrent cell (layers/conv_gru.py:19-28) on the HIP kernels: z = sigmoid(convz([h, x])),
    r = sigmoid(convr([h, x])), q = tanh(convq([r*h, x])), hidden = (1 - z) * h + z * q, the convolutions 3x3 with padding 1 and bias.
    fp32 GPU tensors, 1..64 planes on either side; gradients for last_hidden, x and the six parameters.  return_gates=True returns
    (hidden, z, r, q), the gates detached."""
    args = (last_hidden, x, wz, bz, wr, br, wq, bq)
    if not torch.is_grad_enabled():           # nothing can ask for a gradient: r and q are neither allocated nor stored
        args = tuple(a.detach() for a in args)
    return _ConvGRU.apply(*args, bool(return_gates))


# ---- FeatureDecoder (reference: backbone/TemporalStereo.py:78-90,125-138) ---------------------------------------------------------------
DECODER_MAX_CHANNELS = 512        # the kernel path's envelope: Cu + Cs and Cout (csrc/feature_decoder.hip)


def decoder_conv_supported(in_channels, out_channels):
    return 1 <= in_channels <= DECODER_MAX_CHANNELS and 1 <= out_channels <= DECODER_MAX_CHANNELS


# the 3x3 core's chunked order of a [Cout, Cin, 3, 3] weight
_decoder_weight = _node_weight_layout("decoder", "ts_decoder_weight", "decoder_conv: %d input / %d output channels are outside the kernel path "
                                      + "(1..%d each)" % DECODER_MAX_CHANNELS)


_BN_FOLDS = {}


def _bn_fold(gamma, beta, mean, var, bias, eps, cout):
    """(scale, shift) of an eval-mode BatchNorm folded behind the convolution, from the CURRENT statistics: one ts_bn_fold_many launch
    per call (the one-entry table is uploaded once per layer); inside a `BNFolds` context that context's entry.
    Outside such a context the layer's scale / shift buffers are ONE pair per layer, kept here with its tensors (at most 256 layers, then
    the table starts over) and rewritten by every call: calls of the same layer must be ordered on one stream, as the calls of a module
    are.  Two streams that run the same layer concurrently each need their own `BNFolds` context."""
    if _FOLDS is not None:
        fold = _FOLDS.get(gamma, beta, mean, var, bias, eps, cout)
        if fold is not None:
            return fold
    key = tuple(t.data_ptr() if t is not None else 0 for t in (gamma, beta, mean, var, bias)) + (int(cout),)
    e = _BN_FOLDS.get(key)
    if e is None:
        if len(_BN_FOLDS) >= 256:
            _BN_FOLDS.clear()
        pad = _cpad(cout)
        entry = [gamma, beta, mean, var, bias, torch.empty(pad, device=mean.device), torch.empty(pad, device=mean.device), int(cout), pad]
        e = _BN_FOLDS[key] = (entry, BNFolds()._upload([entry]))
    _lib.check(_lib.lib().ts_bn_fold_many(_lib.ptr(e[1]), 1, float(eps), _stream()), "ts_bn_fold_many")
    return e[0][5], e[0][6]


def _decoder_launch(up, skip, w_l, scale, shift, y, act):
    B, Cout, H, W = y.shape
    Cu, h, w = (up.shape[1], up.shape[2], up.shape[3]) if up is not None else (0, 0, 0)
    Cs = skip.shape[1]
    ub, uc = (up.stride(0), up.stride(1)) if up is not None else (0, 0)
    sb, sc = skip.stride(0), skip.stride(1)
    rc = _lib.lib().ts_decoder_conv_fwd(_lib.ptr(up), _lib.ptr(skip), _lib.ptr(w_l), _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(y), B, Cu, Cs,
                                        Cout, h, w, H, W, int(act), ub, uc, sb, sc, y.stride(0), y.stride(1), _stream())
    _lib.check(rc, "ts_decoder_conv_fwd")


def _decoder_check(up, skip, weight, bias):
    if skip is None:
        raise ValueError("decoder_conv: skip [B,Cs,H,W] is required (it sets the output plane)")
    for name, t in (("up", up), ("skip", skip)):
        if t is not None and t.dim() != 4:
            raise ValueError("decoder_conv: %s must be [B,C,H,W], got %s" % (name, tuple(t.shape)))
    if up is not None and up.shape[0] != skip.shape[0]:
        raise ValueError("decoder_conv: up has batch %d, skip %d" % (up.shape[0], skip.shape[0]))
    Cu = up.shape[1] if up is not None else 0
    Cs = skip.shape[1]
    if weight.dim() != 4 or tuple(weight.shape[1:]) != (Cu + Cs, 3, 3):
        raise ValueError("decoder_conv: weight must be [Cout, %d, 3, 3], got %s" % (Cu + Cs, tuple(weight.shape)))
    if bias is not None and tuple(bias.shape) != (weight.shape[0],):
        raise ValueError("decoder_conv: bias must be [%d], got %s" % (weight.shape[0], tuple(bias.shape)))
    if min(skip.shape) < 1 or (up is not None and min(up.shape) < 1):
        raise ValueError("decoder_conv: empty input")


class _DecoderConv(torch.autograd.Function):
    """act(BatchNorm(conv3x3(cat([resize(up), skip], 1)) + bias)) as ONE autograd node: ts_decoder_conv_fwd reads `up` through the
    align-corners resize and `skip` in place (no resized map, no concatenation), then _bn_act_forward (single rank) over the raw
    convolution output; with may_fold the eval statistics go into the convolution's epilogue and nothing is kept.
    backward: _bn_act_backward -> ts_conv3d_hw_bwd_data over the concatenation's channels, whose [:, Cu:] slice is
    grad_skip as a view and whose [:, :Cu] slice goes through ts_resize_bilinear_bwd -> ts_conv3d_hw_bwd_weight per source and per slice
    of <= 64 output channels (the resized map recomputed by ts_resize_bilinear_fwd) -> ts_channel_sum_fwd.  No atomics."""

    @staticmethod
    def forward(ctx, up, skip, weight, bias, gamma, beta, running_mean, running_var, eps, momentum, act, training, counter, may_fold,
                has_bn):
        _require_gpu(*[t for t in (up, skip, weight, bias) if t is not None])
        _decoder_check(up, skip, weight, bias)
        up = _plane_view(up) if up is not None else None
        skip = _plane_view(skip)
        B, _, H, W = skip.shape
        Cout = weight.shape[0]
        w_l = _decoder_weight(weight)
        y = torch.empty((B, Cout, H, W), device=skip.device, dtype=torch.float32)
        bias_d = _lib.contiguous(bias.detach()) if bias is not None else None
        needs = any(ctx.needs_input_grad[:6])
        if not has_bn:
            if act and needs:
                raise RuntimeError("decoder_conv: an activation without BatchNorm has no backward on the kernel path")
            _decoder_launch(up, skip, w_l, None, bias_d, y, act)
            if needs:
                ctx.save_for_backward(up, skip, weight)
                ctx.meta = (False, 0.0, 0, False, bias is not None)
            return y
        if may_fold and not training:
            scale, shift = _bn_fold(gamma, beta, running_mean, running_var, bias_d, eps, Cout)
            _decoder_launch(up, skip, w_l, scale, shift, y, act)
            return y
        _decoder_launch(up, skip, w_l, None, bias_d, y, 0)
        out, mean, var, _ = _bn_act_forward(y, gamma, beta, running_mean, running_var, eps, momentum, act, training, None, counter)
        if needs:
            ctx.save_for_backward(up, skip, weight, y, mean, var, gamma, beta)
            ctx.meta = (True, float(eps), int(act), bool(training), bias is not None)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        has_bn, eps, act, training, has_bias = ctx.meta
        if has_bn:
            up, skip, weight, y, mean, var, gamma, beta = ctx.saved_tensors
        else:
            up, skip, weight = ctx.saved_tensors
        need = ctx.needs_input_grad
        L, st = _lib.lib(), _stream()
        g = _lib.contiguous(g)
        B, Cout, H, W = g.shape
        N = H * W
        dev = g.device
        ggamma = gbeta = None
        if has_bn:
            dy, s2, s1 = _bn_act_backward(y, g, mean, var, gamma, beta, eps, act, training, None, float(B * N), False)
            ggamma, gbeta = (s2 if need[4] else None), (s1 if need[5] else None)
        else:
            dy = g
        Cu = up.shape[1] if up is not None else 0
        Cs = skip.shape[1]
        Cin = Cu + Cs
        gup = gskip = dw = gbias = None
        if (need[0] and Cu) or need[1]:
            dcat = torch.empty((B, Cin, H, W), device=dev, dtype=torch.float32)
            w_b = _bwd_data_layout(weight, 1, False)
            _lib.check(L.ts_conv3d_hw_bwd_data(_lib.ptr(dy), _lib.ptr(w_b), _lib.ptr(dcat), B, Cin, Cout, 1, H, W, 1, 1, 0, Cout * N, N,
                                               Cin * N, N, st), "ts_conv3d_hw_bwd_data")
            if need[1]:
                gskip = dcat[:, Cu:]
            if need[0] and Cu:
                gup = torch.empty(up.shape, device=dev, dtype=torch.float32)
                _lib.check(L.ts_resize_bilinear_bwd(_lib.ptr(dcat), _lib.ptr(gup), B, Cu, up.shape[2], up.shape[3], H, W, Cin * N, N,
                                                    gup.stride(0), gup.stride(1), st), "ts_resize_bilinear_bwd")
        if need[2]:
            sources = []
            if Cu:
                up_d = _lib.contiguous(up)                  # ts_resize_bilinear_fwd reads a dense map: a sliced `up` is copied HERE (the forward reads it in place)
                resized = torch.empty((B, Cu, H, W), device=dev, dtype=torch.float32)          # recomputed, never kept from the forward
                _lib.check(L.ts_resize_bilinear_fwd(_lib.ptr(up_d), _lib.ptr(resized), B, Cu, up.shape[2], up.shape[3], H, W, 1.0, Cu * N, st),
                           "ts_resize_bilinear_fwd")
                sources.append((resized, Cu))
            sources.append((skip, Cs))
            dw = _wgrad_by_source(sources, dy)
        if has_bias and need[3]:
            gbias = _channel_sum(dy)
        return gup, gskip, dw, gbias, ggamma, gbeta, None, None, None, None, None, None, None, None, None


def bn_exchanges(bn):
    """True when `bn` in its present mode needs other ranks' statistics: a train-mode SyncBatchNorm (anything with a `process_group`)
    whose group spans more than one rank -- the test conv_bn_act applies before it exchanges."""
    if bn is None or not bn.training or "process_group" not in bn.__dict__:
        return False
    import torch.distributed as dist
    return bool(dist.is_available() and dist.is_initialized() and dist.get_world_size(bn.__dict__["process_group"]) > 1)


def decoder_conv(up, skip, weight, bias=None, bn=None, activation=None):
    """One layer of the backbone's decoder on the HIP kernels: activation(bn(conv3x3(cat([resize(up), skip], 1)) + bias)), the resize
    bilinear with align_corners=True to skip's plane, the convolution with stride 1 and padding 1 -- without writing the resized map or
    the concatenation.  up=None is the plain convolution of `skip`; skip is required.  bn: a BatchNorm (train mode: THIS rank's batch
    statistics, the running ones updated; eval mode: the running ones, folded into the convolution's epilogue when nothing needs a
    gradient) or None.  A SyncBatchNorm is accepted in eval mode and on a single rank; in train mode over more than one rank it is
    refused (RuntimeError): the exchange lives in conv_bn_act, which FeatureDecoder._reference_forward goes through.
    activation: None | 'SiLU'.  fp32 GPU tensors, Cu + Cs <= 512, Cout <= 512; gradients for up, skip, weight, bias and bn's affine pair."""
    if activation not in (None, "SiLU"):
        raise ValueError("decoder_conv: activation must be None or 'SiLU'")
    act = BN_ACT[activation]
    if bn is None:
        gamma = beta = rmean = rvar = counter = None
        eps, momentum, training = 0.0, 0.0, False
    else:
        if not isinstance(bn, torch.nn.modules.batchnorm._BatchNorm) or not bn.affine or not bn.track_running_stats:
            raise ValueError("decoder_conv: bn must be a BatchNorm with affine parameters and running statistics")
        if bn.momentum is None:
            raise ValueError("decoder_conv: a BatchNorm with momentum=None (cumulative average) is not on the kernel path")
        if bn_exchanges(bn):
            raise RuntimeError("decoder_conv: a train-mode SyncBatchNorm over %d ranks needs the statistics exchange of conv_bn_act; "
                               "this node computes per-rank statistics (FeatureDecoder routes such a module to _reference_forward)"
                               % torch.distributed.get_world_size(bn.__dict__["process_group"]))
        gamma, beta, rmean, rvar = bn.weight, bn.bias, bn.running_mean, bn.running_var
        training = bn.training
        eps, momentum = bn.eps, bn.momentum
        counter = bn.num_batches_tracked if training else None
    tensors = (up, skip, weight, bias, gamma, beta)
    grad = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)
    if not grad:
        tensors = tuple(t.detach() if t is not None else None for t in tensors)
    return _DecoderConv.apply(*tensors, rmean, rvar, eps, momentum, act, training, counter, not grad, bn is not None)


# ---- MemoryInvertedResidual (reference: backbone/TemporalStereo.py:165-218) ------------------------------------------------------------
MBCONV_MAX_CHANNELS = 512         # the kernel path's envelope (csrc/mbconv.hip): the block's width C and the squeeze width Cr ...
MBCONV_MAX_MID = 2048             # ... and the expanded width Cmid


def mbconv_supported(C, Cmid, Cr):
    return 1 <= C <= MBCONV_MAX_CHANNELS and 1 <= Cmid <= MBCONV_MAX_MID and 1 <= Cr <= MBCONV_MAX_CHANNELS


# the pointwise core's order of a [Cout, Cin, 1, 1] weight
_mbconv_weight = _node_weight_layout("mbconv", "ts_mbconv_weight", "mbconv: a 1x1 weight of %d input / %d output channels is outside the kernel path "
                                     + "(1..%d each)" % MBCONV_MAX_MID)


def _bn_eval_fold(bn, bias=None):
    """(scale, shift) of an eval-mode BatchNorm behind a convolution: `_bn_fold`'s entry (a `BNFolds` context's when one is open)."""
    return _bn_fold(bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var, bias, bn.eps, bn.num_features)


def _depthwise_launch(x, w9, scale, shift, y, plane_sum, act, flip):
    B, C, H, W = x.shape
    rc = _lib.lib().ts_depthwise3x3_fwd(_lib.ptr(x), _lib.ptr(w9), _lib.ptr(scale), _lib.ptr(shift), _lib.ptr(y), _lib.ptr(plane_sum), B, C, H,
                                        W, int(act), int(flip), x.stride(0), x.stride(1), y.stride(0), y.stride(1), _stream())
    _lib.check(rc, "ts_depthwise3x3_fwd")


def _mbconv_check(inp, memory, w_pw, fold1, w_dw, fold2, w_reduce, b_reduce, w_expand, b_expand, w_pwl, fold3, out):
    """Shapes of everything mbconv_eval hands to the kernels, before any launch: they take B, H and W from `inp` alone."""
    if inp.dim() != 4 or min(inp.shape) < 1:
        raise ValueError("mbconv_eval: input must be a non-empty [B,C,H,W], got %s" % (tuple(inp.shape),))
    B, C, H, W = inp.shape
    if w_pw.dim() != 4 or tuple(w_pw.shape[1:]) != (C, 1, 1):
        raise ValueError("mbconv_eval: conv_pw weight must be [Cmid, %d, 1, 1], got %s" % (C, tuple(w_pw.shape)))
    Cmid = w_pw.shape[0]
    if w_reduce.dim() != 4 or tuple(w_reduce.shape[1:]) != (Cmid, 1, 1):
        raise ValueError("mbconv_eval: conv_reduce weight must be [Cr, %d, 1, 1], got %s" % (Cmid, tuple(w_reduce.shape)))
    Cr = w_reduce.shape[0]
    for name, t, shape in (("conv_dw weight", w_dw, (Cmid, 1, 3, 3)), ("conv_reduce bias", b_reduce, (Cr,)),
                           ("conv_expand weight", w_expand, (Cmid, Cr, 1, 1)), ("conv_expand bias", b_expand, (Cmid,)),
                           ("conv_pwl weight", w_pwl, (C, Cmid, 1, 1))):
        if t is None or tuple(t.shape) != shape:
            raise ValueError("mbconv_eval: %s must be %s, got %s" % (name, list(shape), None if t is None else tuple(t.shape)))
    for name, fold, n in (("bn1", fold1, Cmid), ("bn2", fold2, Cmid), ("bn3", fold3, C)):
        _fold_check("mbconv_eval", name, fold, n, required=True)
    if not mbconv_supported(C, Cmid, Cr):
        raise RuntimeError("mbconv_eval: C = %d, Cmid = %d, Cr = %d are outside the kernel path (C, Cr <= %d, Cmid <= %d)"
                           % (C, Cmid, Cr, MBCONV_MAX_CHANNELS, MBCONV_MAX_MID))
    if memory is not None:
        if memory.dim() != 4 or memory.shape[0] != B or tuple(memory.shape[2:]) != (H, W) or not 1 <= memory.shape[1] <= C:
            raise ValueError("mbconv_eval: memory must be [%d, mc <= %d, %d, %d] as the input is %s, got %s"
                             % (B, C, H, W, tuple(inp.shape), tuple(memory.shape)))
    if out is not None:
        _out_check("mbconv_eval", "out", out, (B, C, H, W))


def mbconv_eval(inp, memory, w_pw, fold1, w_dw, fold2, w_reduce, b_reduce, w_expand, b_expand, w_pwl, fold3, out=None,
                return_stages=False):
    """The eval form of one MemoryInvertedResidual block as FOUR launches (csrc/mbconv.hip): expand (reads [memory | inp[:, mc:]] in
    place), depthwise (+ the plane sums), gate, project (reads the gated map, adds `inp`).  fold1..3: (scale, shift) of the three
    BatchNorms (`_bn_eval_fold`); the weights as the framework holds them; memory [B,mc,H,W] or None.  Nothing here asks for a
    gradient: the caller has checked.  Outside `WeightLayouts` / `BNFolds` contexts the two weight layouts and three folds are launches
    of their own.  -> the block's output [B,C,H,W] (written into `out` when given); with return_stages also (after act1, after act2,
    gate)."""
    _mbconv_check(inp, memory, w_pw, fold1, w_dw, fold2, w_reduce, b_reduce, w_expand, b_expand, w_pwl, fold3, out)
    _require_gpu(inp, memory, w_pw, w_dw, w_reduce, b_reduce, w_expand, b_expand, w_pwl, out, *fold1, *fold2, *fold3)
    inp = _plane_view(inp)
    B, C, H, W = inp.shape
    Cmid, Cr = w_pw.shape[0], w_reduce.shape[0]
    memory, mb, mcs = _optional_operand(memory)
    mc = memory.shape[1] if memory is not None else 0
    dev = inp.device
    L, st = _lib.lib(), _stream()
    e = torch.empty((B, Cmid, H, W), device=dev, dtype=torch.float32)
    rc = L.ts_mbconv_expand_fwd(_lib.ptr(memory), _lib.ptr(inp), _lib.ptr(_mbconv_weight(w_pw)), _lib.ptr(fold1[0]), _lib.ptr(fold1[1]),
                                _lib.ptr(e), B, C, mc, Cmid, H, W, mb, mcs, inp.stride(0), inp.stride(1), Cmid * H * W, H * W, st)
    _lib.check(rc, "ts_mbconv_expand_fwd")
    d = torch.empty_like(e)
    sums = torch.empty((B, Cmid), device=dev, dtype=torch.float32)
    _depthwise_launch(e, _lib.contiguous(w_dw.detach()), fold2[0], fold2[1], d, sums, 1, 0)
    gate = torch.empty((B, Cmid), device=dev, dtype=torch.float32)
    rc = L.ts_se_gate_fwd(_lib.ptr(sums), _lib.ptr(_lib.contiguous(w_reduce.detach())), _lib.ptr(b_reduce.detach()),
                          _lib.ptr(_lib.contiguous(w_expand.detach())), _lib.ptr(b_expand.detach()), _lib.ptr(gate), B, Cmid, Cr,
                          1.0 / float(H * W), st)
    _lib.check(rc, "ts_se_gate_fwd")
    y = torch.empty((B, C, H, W), device=dev, dtype=torch.float32) if out is None else out
    rc = L.ts_mbconv_project_fwd(_lib.ptr(d), _lib.ptr(gate), _lib.ptr(_mbconv_weight(w_pwl)), _lib.ptr(fold3[0]), _lib.ptr(fold3[1]),
                                 _lib.ptr(inp), _lib.ptr(y), B, Cmid, C, H, W, Cmid * H * W, H * W, inp.stride(0), inp.stride(1), y.stride(0),
                                 y.stride(1), st)
    _lib.check(rc, "ts_mbconv_project_fwd")
    return (y, e, d, gate) if return_stages else y


class _Depthwise3x3(torch.autograd.Function):
    """conv2d(x, weight [C,1,3,3], bias, stride 1, padding 1, groups C) on csrc/mbconv.hip: ts_depthwise3x3_fwd (the bias is its
    epilogue's shift); backward: the same entry with the taps flipped over dy (input gradient), ts_depthwise3x3_bwd_weight, and
    ts_channel_sum_fwd for the bias.  No atomics."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        _require_gpu(x, weight, bias)
        if x.dim() != 4 or weight.dim() != 4 or tuple(weight.shape) != (x.shape[1], 1, 3, 3):
            raise ValueError("depthwise_conv3x3: x [B,C,H,W] and weight [C,1,3,3] expected, got %s and %s" % (tuple(x.shape), tuple(weight.shape)))
        if bias is not None and tuple(bias.shape) != (x.shape[1],):
            raise ValueError("depthwise_conv3x3: bias must be [%d], got %s" % (x.shape[1], tuple(bias.shape)))
        if min(x.shape) < 1:
            raise ValueError("depthwise_conv3x3: empty input")
        x = _plane_view(x)
        w9 = _lib.contiguous(weight.detach())
        y = torch.empty(x.shape, device=x.device, dtype=torch.float32)
        _depthwise_launch(x, w9, None, _lib.contiguous(bias.detach()) if bias is not None else None, y, None, 0, 0)
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        need = ctx.needs_input_grad
        g = _plane_view(g)
        B, C, H, W = g.shape
        gx = gw = gb = None
        if need[0]:
            gx = torch.empty((B, C, H, W), device=g.device, dtype=torch.float32)
            _depthwise_launch(g, _lib.contiguous(weight.detach()), None, None, gx, None, 0, 1)
        if need[1]:
            gw = torch.empty(weight.shape, device=g.device, dtype=torch.float32)
            rc = _lib.lib().ts_depthwise3x3_bwd_weight(_lib.ptr(x), _lib.ptr(g), _lib.ptr(gw), B, C, H, W, x.stride(0), x.stride(1),
                                                       g.stride(0), g.stride(1), _stream())
            _lib.check(rc, "ts_depthwise3x3_bwd_weight")
        if ctx.has_bias and need[2]:
            gb = _channel_sum(g)
        return gx, gw, gb


def depthwise_conv3x3(x, weight, bias=None):
    """F.conv2d(x, weight, bias, stride=1, padding=1, groups=C) for a [C,1,3,3] weight on the HIP kernels (fp32 GPU tensors; any plane),
    with gradients for x, weight and bias."""
    return _Depthwise3x3.apply(x, weight, bias)


# ---- the encoder's large planes: stem, ConvBnAct, fused MBConv (reference: backbone/TemporalStereo.py:62-70,105-113) --------------------
CONV3X3_S_MAX_CHANNELS = 512      # the kernel path's envelope (csrc/fused_mbconv.hip): the 3x3's core channels -- Cin at stride 1, 4 Cin at
#                                   stride 2 (the phase form) -- and its Cout; the projection takes Cmid <= 2048 and Cout <= 512


def conv3x3_s_supported(Cin, Cout, stride):
    return stride in (1, 2) and 1 <= Cin and Cin * (4 if stride == 2 else 1) <= CONV3X3_S_MAX_CHANNELS and 1 <= Cout <= CONV3X3_S_MAX_CHANNELS


def fused_mbconv_supported(Cin, Cmid, Cout, stride):
    """Whether a fused (edge-residual) block Cin -> Cmid (3x3, stride 1 | 2) -> Cout (1x1) is inside the kernels' envelope."""
    return conv3x3_s_supported(Cin, Cmid, stride) and 1 <= Cmid <= MBCONV_MAX_MID and 1 <= Cout <= MBCONV_MAX_CHANNELS


# the 3x3 core's chunked order of a [Cout, Cin, 3, 3] weight for one stride (at stride 2 the phase order)
_CONV3X3_S_WEIGHT = {stride: _node_weight_layout("conv3x3_s%d" % stride, "ts_conv3x3_s_weight",
                                                 "conv3x3_bn_act: %d input / %d output channels at stride %d are outside the kernel path "
                                                 + "(4 Cin <= %d at stride 2, Cin and Cout <= %d)" % ((CONV3X3_S_MAX_CHANNELS,) * 2), stride)
                     for stride in (1, 2)}


def conv3x3_bn_act(x, weight, fold, stride, activation, residual=None, out=None):
    """The eval form of a 3x3 convolution (padding 1, stride 1 | 2, no bias) with its BatchNorm folded, its activation and -- at stride 1 --
    a residual added AFTER the activation, as ONE launch (csrc/fused_mbconv.hip, ts_conv3x3_s_fwd): the reference encoder's stem, a
    ConvBnAct of block0, the expansion of a fused block.  x [B,Cin,H,W] is read in place through its strides; weight [Cout,Cin,3,3] as the
    framework holds it; fold: (scale, shift) of the BatchNorm (`_bn_eval_fold`) or None; activation None | 'SiLU'; residual
    [B,Cout,H,W] or None.  -> [B,Cout,ceil(H/s),ceil(W/s)] (written into `out` when given).  Nothing here asks for a gradient: the caller
    has checked.  Outside a `WeightLayouts` context the weight layout is a launch of its own."""
    what = "conv3x3_bn_act"
    if activation not in (None, "SiLU"):
        raise ValueError("%s: activation must be None or 'SiLU'" % what)
    if stride not in (1, 2):
        raise ValueError("%s: stride must be 1 or 2, got %r" % (what, stride))
    if x.dim() != 4 or min(x.shape) < 1:
        raise ValueError("%s: x must be a non-empty [B,C,H,W], got %s" % (what, tuple(x.shape)))
    B, Cin, H, W = x.shape
    if weight.dim() != 4 or tuple(weight.shape[1:]) != (Cin, 3, 3):
        raise ValueError("%s: weight must be [Cout, %d, 3, 3], got %s" % (what, Cin, tuple(weight.shape)))
    Cout = weight.shape[0]
    scale, shift = _fold_check(what, "BatchNorm", fold, Cout)
    if not conv3x3_s_supported(Cin, Cout, stride):
        raise RuntimeError("%s: %d input / %d output channels at stride %d are outside the kernel path" % (what, Cin, Cout, stride))
    Ho, Wo = (H + stride - 1) // stride, (W + stride - 1) // stride
    if residual is not None:
        if stride != 1:
            raise ValueError("%s: a residual is taken at stride 1 only" % what)
        if tuple(residual.shape) != (B, Cout, Ho, Wo):
            raise ValueError("%s: residual must be %s, got %s" % (what, [B, Cout, Ho, Wo], tuple(residual.shape)))
    if out is not None:
        _out_check(what, "out", out, (B, Cout, Ho, Wo))
    _require_gpu(x, weight, scale, shift, residual, out)
    x = _plane_view(x)
    residual, rb, rc = _optional_operand(residual)
    y = torch.empty((B, Cout, Ho, Wo), device=x.device, dtype=torch.float32) if out is None else out
    code = _lib.lib().ts_conv3x3_s_fwd(_lib.ptr(x), _lib.ptr(_CONV3X3_S_WEIGHT[stride](weight)), _lib.ptr(scale), _lib.ptr(shift),
                                       _lib.ptr(residual), _lib.ptr(y), B, Cin, Cout, H, W, int(stride), BN_ACT[activation], x.stride(0),
                                       x.stride(1), rb, rc, y.stride(0), y.stride(1), _stream())
    _lib.check(code, "ts_conv3x3_s_fwd")
    return y


def fused_mbconv_eval(x, w_exp, fold1, stride, w_pwl, fold2, residual, out=None, return_stages=False):
    """The eval form of one fused (edge-residual) block as TWO launches (csrc/fused_mbconv.hip): the 3x3 expansion with bn1 and SiLU
    (`conv3x3_bn_act`; it writes the mid map [B,Cmid,ceil(H/s),ceil(W/s)]) and the 1x1 projection that folds bn2 and adds the residual
    (ts_fused_project_fwd).  fold1 / fold2: (scale, shift) of the two BatchNorms (`_bn_eval_fold`); the weights as the framework holds
    them; residual: the tensor added to the projection ([B,Cout,.,.], for a residual block the input itself) or None.  Nothing here asks
    for a gradient: the caller has checked.  Outside `WeightLayouts` / `BNFolds` contexts the two weight layouts and two folds are
    launches of their own.  -> the block's output (written into `out` when given); with return_stages also the mid map."""
    what = "fused_mbconv_eval"
    if x.dim() != 4 or min(x.shape) < 1:
        raise ValueError("%s: x must be a non-empty [B,C,H,W], got %s" % (what, tuple(x.shape)))
    if w_exp.dim() != 4 or w_pwl.dim() != 4 or tuple(w_pwl.shape[1:]) != (w_exp.shape[0], 1, 1):
        raise ValueError("%s: conv_exp weight [Cmid,Cin,3,3] and conv_pwl weight [Cout,Cmid,1,1] expected, got %s and %s"
                         % (what, tuple(w_exp.shape), tuple(w_pwl.shape)))
    B, Cin, H, W = x.shape
    Cmid, Cout = w_exp.shape[0], w_pwl.shape[0]
    if fold1 is None or fold2 is None:
        raise ValueError("%s: both BatchNorm folds are required" % what)
    scale2, shift2 = _fold_check(what, "bn2", fold2, Cout)
    if stride not in (1, 2) or not fused_mbconv_supported(Cin, Cmid, Cout, stride):
        raise RuntimeError("%s: Cin = %d, Cmid = %d, Cout = %d at stride %r are outside the kernel path" % (what, Cin, Cmid, Cout, stride))
    Ho, Wo = (H + stride - 1) // stride, (W + stride - 1) // stride
    if residual is not None and tuple(residual.shape) != (B, Cout, Ho, Wo):
        raise ValueError("%s: residual must be %s, got %s" % (what, [B, Cout, Ho, Wo], tuple(residual.shape)))
    if out is not None:
        _out_check(what, "out", out, (B, Cout, Ho, Wo))
    _require_gpu(w_pwl, scale2, shift2, residual, out)
    mid = conv3x3_bn_act(x, w_exp, fold1, stride, "SiLU")
    residual, rb, rc = _optional_operand(residual)
    y = torch.empty((B, Cout, Ho, Wo), device=x.device, dtype=torch.float32) if out is None else out
    code = _lib.lib().ts_fused_project_fwd(_lib.ptr(mid), _lib.ptr(_mbconv_weight(w_pwl)), _lib.ptr(scale2), _lib.ptr(shift2),
                                           _lib.ptr(residual), _lib.ptr(y), B, Cmid, Cout, Ho, Wo, mid.stride(0), mid.stride(1), rb, rc,
                                           y.stride(0), y.stride(1), _stream())
    _lib.check(code, "ts_fused_project_fwd")
    return (y, mid) if return_stages else y
