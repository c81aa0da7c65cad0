"""Disparity and error colour maps and the 16-bit disparity map on the device, on the kernels of csrc/render.hip.

Drop-ins with the reference's names and argument order (architecture/utils/visualization/disparity_colormap.py):
  disp_to_color            :69-98   (disp_map :5-66)
  disp_err_to_color        :102-170
  disp_err_to_colorbar     :172-219 (revalue :172-178)
  colormap                 architecture/utils/visualization/colormap.py:5-85, the callable form only
plus `disp_to_uint16`, the KITTI submission form `(disp * 256).astype('uint16')` (projects/TemporalStereo/video_inference.py:220),
and `render_frame`, the fused form of what `visualize` (video_inference.py:169-227) does with a frame: the rescale to the ground
truth's size (:182), the estimate coloured above the ground truth with one shared maximum (:201-202), both error maps (:203-204)
and the 16-bit map, in one statistics launch pair and one colour launch for the whole batch.

Semantics kept from the reference:
  - disp_to_color scales by the map's own maximum unless one is given, and does not clip: values below 0 and above the maximum
    extrapolate the first / last segment of the colour ramp (`clip=True` gives what the reference's callers apply afterwards);
  - disp_err_to_color as written: both maps are multiplied by 255 first, so the absolute branch is 255 |e| / 3 while the relative
    one is |e| / gt / 0.05; the ten classes are closed on both ends and a later class wins a shared end point; gt <= 0 stays black;
  - disp_err_to_colorbar: the error |est - gt| * (gt > 0) of each of the ranges (0,1] (1,2] (2,4] (4,12] (12,16]
    (16, max(192, max error)] is spread over the range's share of [0,1] between the range's own minimum and maximum, the product
    with the share taken in float64 and rounded to float32 as numpy >= 2 does, then matplotlib's 256-entry jet; a NaN is black (the
    colour map's `bad` colour), and a NaN anywhere in the error makes the last range (16, 192] as Python's max(192, nan) does;
  - non-finite values propagate as numpy propagates them: a NaN in the map makes its maximum NaN and every colour NaN.
Differences, deliberate:
  - inputs are fp32 GPU tensors, [H,W] or batched [B,H,W] / [B,1,H,W] with one maximum and one set of ranges PER IMAGE; results are
    tensors ON THE DEVICE, float32 where the reference returns float64 (the colour ramp is interpolated in fp32: within 5e-6 of the
    reference), or uint8 = floor(255 v + 0.5) after a clamp to [0,1] with NaN -> 0 (`dtype=torch.uint8`), HWC or CHW;
  - nothing here synchronises with the host; `max_disp` may be a [B] device tensor so that a maximum found on the device stays there;
  - disp_to_uint16 truncates toward zero as numpy's cast does for values in [0, 65536 / scale); outside that range numpy's result
    depends on the platform, here the map saturates to [0, 65535] and a NaN becomes 0;
  - only the `jet` colour map; matplotlib is not imported, the table is rebuilt from jet's published segment data.
fp32 GPU tensors only: a CPU tensor raises, there is no CPU fallback.

Optical flow, on the kernels of csrc/flow_frame.hip -- drop-ins with the reference's names and argument order
(architecture/utils/visualization/flow_colormap.py):
  make_color_wheel         :8-56    (host, numpy: the 55 x 3 table, uploaded once per device)
  flow_max_rad             :59-77
  flow_color, flow_to_color  :80-167  (the two differ only in how they blacken unknown pixels; the results are equal)
  flow_err_to_color        :170-220
plus `render_flow_frame`, the fused form: the estimate at its native resolution read through the align-corners rescale to the
ground truth's size, coloured above the ground truth with one shared maximum radius, and the error classes, in one statistics
launch pair and one colour launch for the whole batch.
Semantics kept from the reference:
  - unknown pixels (|u| or |v| > 1e7, or NaN) count as (0, 0) in the maximum radius and come out black;
  - u, v are divided by max_rad + 2^-52 in fp32; the angle is atan2(-v, -u) / pi with the true signs of its arguments, signed zeros
    included (the wheel does not close: at u > 0 the colour jumps with the sign of v); fk = (a + 1) / 2 * 54 + 1, k1 wraps to 1 at 56;
    rad <= 1: 1 - rad (1 - col), else 0.75 col;
  - flow_err_to_color: E = sqrt(|F_gt - F_est|^2) * F_gt_val in fp32, ten classes closed on both ends, a later class wins a shared
    end point; F_gt_val == 0 and a NaN E are black.
Differences, deliberate:
  - inputs are fp32 GPU tensors in the reference's layout [H,W,2] / batched [B,H,W,2] (`layout='HWC'`) or [2,H,W] / [B,2,H,W]
    (`layout='CHW'`), read in place either way, with one maximum PER IMAGE; inputs are never modified (the reference zeroes the
    unknown pixels in the caller's array);
  - results are device tensors, float32 (the wheel is interpolated in fp32 where the reference uses float64) or uint8, HWC or CHW;
  - with a maximum taken from the data, "inside the disc" is decided on the unnormalised radius r <= max_rad, so the brightest
    pixel is never darkened by the rounding of u / max_rad (in the reference it can be); with a given maximum the normalised radius
    decides, as in the reference;
  - the angle is evaluated in fp64 and rounded once; `max_rad` may be a number or a [B] device tensor; a NaN maximum gives NaN
    colours where the reference raises.
"""
import numpy as np
import torch

from . import _lib
from .functional import _require_gpu, _stream

# flag word of ts_disp_render_fwd (include/ts_hip.h)
EST_COLOR, GT_COLOR, ERR_CLASS, ERR_JET, U16, UINT8, CHW, BAR, CLIP, MAX_SHARED, MAX_GIVEN = (1 << i for i in range(11))
STATS_FLOATS = 32
BAR_ROWS = 50
OUTPUTS = ('disp_color', 'error_map', 'error_bar_map', 'disp_u16')

# flag word of ts_flow_render_fwd (include/ts_hip.h)
(FLOW_EST_COLOR, FLOW_GT_COLOR, FLOW_ERR_CLASS, FLOW_STATS, FLOW_UINT8, FLOW_CHW, FLOW_MAX_SHARED, FLOW_MAX_GIVEN, FLOW_EST_HWC,
 FLOW_GT_HWC) = (1 << i for i in range(10))
FLOW_STATS_FLOATS = 16
FLOW_OUTPUTS = ('flow_color', 'error_map')
_WHEEL = {}

# matplotlib's `jet` (its _jet_data): per channel the break points (x, value below, value above) of a piecewise-linear ramp
_JET_SEGMENTS = {
    'red': ((0.00, 0, 0), (0.35, 0, 0), (0.66, 1, 1), (0.89, 1, 1), (1.00, 0.5, 0.5)),
    'green': ((0.000, 0, 0), (0.125, 0, 0), (0.375, 1, 1), (0.640, 1, 1), (0.910, 0, 0), (1.000, 0, 0)),
    'blue': ((0.00, 0.5, 0.5), (0.11, 1, 1), (0.34, 1, 1), (0.65, 0, 0), (1.00, 0, 0)),
}
_JET = {}


def jet_table(n=256):
    """The n x 3 float32 lookup table of `jet`: the segment data sampled at linspace(0, 1, n), as a LinearSegmentedColormap does."""
    xs = np.linspace(0.0, 1.0, n)
    lut = np.empty((n, 3), dtype=np.float64)
    for c, name in enumerate(('red', 'green', 'blue')):
        seg = np.array(_JET_SEGMENTS[name], dtype=np.float64)
        x, y0, y1 = seg[:, 0], seg[:, 1], seg[:, 2]
        ind = np.searchsorted(x, xs)[1:-1]
        dist = (xs[1:-1] - x[ind - 1]) / (x[ind] - x[ind - 1])
        lut[:, c] = np.concatenate([[y1[0]], dist * (y0[ind] - y1[ind - 1]) + y1[ind - 1], [y0[-1]]])
    return np.clip(lut, 0.0, 1.0).astype(np.float32)


def _jet(device):
    key = (device.type, device.index)
    if key not in _JET:
        _JET[key] = torch.from_numpy(jet_table()).to(device).contiguous()
    return _JET[key]


def _maps(what, *tensors):
    """[H,W] / [B,H,W] / [B,1,H,W] maps of one batch -> contiguous tensors, B, their sizes, and whether a batch axis is returned."""
    _require_gpu(*tensors)
    first = tensors[0]
    out, sizes = [], []
    for t in tensors:
        if t is None:
            out.append(None)
            sizes.append(None)
            continue
        if t.dim() not in (2, 3, 4) or (t.dim() == 4 and t.shape[1] != 1) or t.dim() != first.dim():
            raise ValueError("%s: maps must be [H,W], [B,H,W] or [B,1,H,W], all of one rank (got %s)"
                             % (what, [tuple(x.shape) for x in tensors if x is not None]))
        if t.dim() > 2 and t.shape[0] != first.shape[0]:
            raise ValueError("%s: batch sizes differ (%d and %d)" % (what, first.shape[0], t.shape[0]))
        if t.numel() == 0:
            raise ValueError("%s: empty map of shape %s" % (what, tuple(t.shape)))
        out.append(_lib.contiguous(t))
        sizes.append(tuple(t.shape[-2:]))
    return out, (1 if first.dim() == 2 else first.shape[0]), sizes, first.dim() > 2


def _fmt(dtype, format):
    if dtype not in (torch.float32, torch.uint8):
        raise ValueError("dtype must be torch.float32 or torch.uint8 (got %s)" % (dtype,))
    if format not in ('HWC', 'CHW'):
        raise ValueError(format)
    return (UINT8 if dtype == torch.uint8 else 0) | (CHW if format == 'CHW' else 0)


def _render(est, gt, hw, B, size, flags, max_disp=None, scale=256.0, batched=True, dtype=torch.float32, format='HWC'):
    """One ts_disp_render_fwd call.  Returns {'disp_color', 'err_class', 'err_jet', 'u16', 'stats'}: those that flags selects."""
    dev = est.device
    Hg, Wg = size
    L = _lib.lib()
    res = {}

    def color(rows):
        shape = (B, 3, rows, Wg) if format == 'CHW' else (B, rows, Wg, 3)
        return torch.empty(shape, device=dev, dtype=dtype)
    if flags & (EST_COLOR | GT_COLOR):
        res['disp_color'] = color(2 * Hg if (flags & EST_COLOR) and (flags & GT_COLOR) else Hg)
    if flags & ERR_CLASS:
        res['err_class'] = color(Hg)
    if flags & ERR_JET:
        res['err_jet'] = color(Hg + (BAR_ROWS if flags & BAR else 0))
    if flags & U16:
        res['u16'] = torch.empty((B, Hg, Wg), device=dev, dtype=torch.int16).view(torch.uint16)
    maxd = None
    if max_disp is not None and flags & (EST_COLOR | GT_COLOR):
        if torch.is_tensor(max_disp):
            _require_gpu(max_disp)
            if max_disp.numel() != B:
                raise ValueError("max_disp must hold one maximum per image (%d), got shape %s" % (B, tuple(max_disp.shape)))
            maxd = _lib.contiguous(max_disp.reshape(B))
        else:
            maxd = torch.full((B,), float(max_disp), device=dev, dtype=torch.float32)
        flags |= MAX_GIVEN
    stats = ws = None
    if flags & ERR_JET or (flags & (EST_COLOR | GT_COLOR) and maxd is None):
        stats = torch.empty((B, STATS_FLOATS), device=dev, dtype=torch.float32)
        ws = torch.empty(int(L.ts_disp_render_workspace_bytes(B, Hg, Wg)), device=dev, dtype=torch.uint8)
        res['stats'] = stats
    jet = _jet(dev) if flags & ERR_JET else None
    _lib.check(L.ts_disp_render_fwd(_lib.ptr(est), _lib.ptr(gt), _lib.ptr(maxd), _lib.ptr(jet), B, hw[0], hw[1], Hg, Wg, flags,
                                    float(scale), _lib.ptr(res.get('disp_color')), _lib.ptr(res.get('err_class')),
                                    _lib.ptr(res.get('err_jet')), _lib.ptr(res.get('u16')), _lib.ptr(stats), _lib.ptr(ws), _stream()),
               "ts_disp_render_fwd")
    if not batched:
        res = {k: (v[0] if k != 'stats' else v) for k, v in res.items()}
    return res


def disp_to_color(disp, max_disp=None, clip=False, dtype=torch.float32, format='HWC'):
    """disparity_colormap.py:69-98: the KITTI disparity colours of disp ([H,W] -> [H,W,3]; [B,H,W] / [B,1,H,W] -> [B,H,W,3]).
    max_disp: None (each image's own maximum, found on the device), a number, or a [B] device tensor.  Not clipped unless clip."""
    (d,), B, (hw,), batched = _maps("disp_to_color", disp)
    flags = EST_COLOR | (CLIP if clip else 0) | _fmt(dtype, format)
    return _render(d, None, hw, B, hw, flags, max_disp=max_disp, batched=batched, dtype=dtype, format=format)['disp_color']


def disp_err_to_color(disp_est, disp_gt, dtype=torch.float32, format='HWC'):
    """disparity_colormap.py:102-170: the KITTI error classes of disp_est against disp_gt (one shape)."""
    (e, g), B, (hw, ghw), batched = _maps("disp_err_to_color", disp_est, disp_gt)
    if hw != ghw:
        raise ValueError("disp_est has shape %s, disp_gt %s" % (tuple(disp_est.shape), tuple(disp_gt.shape)))
    return _render(e, g, hw, B, hw, ERR_CLASS | _fmt(dtype, format), batched=batched, dtype=dtype, format=format)['err_class']


def disp_err_to_colorbar(est, gt, with_bar=False, cmap='jet', dtype=torch.float32, format='HWC'):
    """disparity_colormap.py:172-219: the absolute error through six data-dependent ranges and jet; with_bar appends the 50-row
    legend ([H+50,W,3]).  Only cmap='jet'."""
    if cmap != 'jet':
        raise ValueError("only the 'jet' colour map is built in (got %r)" % (cmap,))
    (e, g), B, (hw, ghw), batched = _maps("disp_err_to_colorbar", est, gt)
    if hw != ghw:
        raise ValueError("est has shape %s, gt %s" % (tuple(est.shape), tuple(gt.shape)))
    flags = ERR_JET | (BAR if with_bar else 0) | _fmt(dtype, format)
    return _render(e, g, hw, B, hw, flags, batched=batched, dtype=dtype, format=format)['err_jet']


def disp_to_uint16(disp, scale=256):
    """(disp * scale).astype('uint16') (video_inference.py:220) as a torch.uint16 tensor of disp's spatial shape ([B,1,H,W] ->
    [B,H,W]): truncated toward zero as numpy's cast does for values in [0, 65536 / scale).  Outside that range numpy's result
    depends on the platform; here the map SATURATES to [0, 65535], and a NaN becomes 0."""
    (d,), B, (hw,), batched = _maps("disp_to_uint16", disp)
    return _render(d, None, hw, B, hw, U16, scale=scale, batched=batched)['u16']


def render_stats(est, gt=None, size=None):
    """The per-image statistics the colour launch reads, [B, 32] fp32 on the device (layout: include/ts_hip.h), of est rescaled
    to gt's size (or `size`): maxima of est / gt / both / the error, and per range the error's minimum, maximum and count."""
    (e, g), B, (hw, ghw), _ = _maps("render_stats", est, gt)
    size = _target(hw, ghw, size)
    flags = (ERR_JET if g is not None else EST_COLOR)
    return _render(e, g, hw, B, size, flags)['stats']


def range_counts(stats):
    """The members' counts of the six ranges, [B, 6] int32, out of a render_stats tensor."""
    return stats[:, 24:30].contiguous().view(torch.int32)


def _target(hw, ghw, size):
    if ghw is not None:
        if size is not None and tuple(size) != ghw:
            raise ValueError("size %s differs from the ground truth's %s" % (tuple(size), ghw))
        return ghw
    return tuple(int(v) for v in size) if size is not None else hw


def render_frame(disp, gt=None, size=None, outputs=None, dtype=torch.uint8, format='HWC', clip=True, scale=256):
    """The pictures `visualize` (video_inference.py:169-227) makes of a frame, fused: disp at its NATIVE resolution ([B,1,h,w],
    [B,h,w] or [h,w]) is read through the align-corners rescale to gt's size (or `size`; value-scaled by W / w, :182) and never
    written at full size.  Returns a dict of device tensors, those of `outputs` (default: all that apply):
      'disp_color'     the estimate's disparity colours above the ground truth's, one shared maximum per image (:201-202),
                       [B,2H,W,3]; without gt the estimate alone with its own maximum, [B,H,W,3] (:207-208)
      'error_map'      disp_err_to_color (:203)                                         needs gt
      'error_bar_map'  disp_err_to_colorbar(with_bar=True, cmap='jet'), [B,H+50,W,3] (:204)   needs gt
      'disp_u16'       disp_to_uint16 of the rescaled estimate, [B,H,W] (:220)
    clip: the `.clip(0, 1)` visualize applies to every picture (the error maps are inside [0,1] anyway).
    One statistics launch pair and one colour launch for the whole dict, batched over B."""
    (e, g), B, (hw, ghw), batched = _maps("render_frame", disp, gt)
    size = _target(hw, ghw, size)
    if outputs is None:
        outputs = OUTPUTS if g is not None else ('disp_color', 'disp_u16')
    flags = _fmt(dtype, format) | (CLIP if clip else 0)
    for o in outputs:
        if o not in OUTPUTS:
            raise ValueError("unknown output %r (one of %s)" % (o, OUTPUTS))
        if g is None and o in ('error_map', 'error_bar_map'):
            raise ValueError("%s needs a ground truth" % o)
        flags |= {'disp_color': EST_COLOR | (GT_COLOR | MAX_SHARED if g is not None else 0), 'error_map': ERR_CLASS,
                  'error_bar_map': ERR_JET | BAR, 'disp_u16': U16}[o]
    if not outputs:
        return {}
    r = _render(e, g, hw, B, size, flags, scale=scale, batched=batched, dtype=dtype, format=format)
    names = {'disp_color': 'disp_color', 'error_map': 'err_class', 'error_bar_map': 'err_jet', 'disp_u16': 'u16'}
    return {o: r[names[o]] for o in outputs}


def colormap(_cmap, *args, normalize=False, format='HWC', **kwargs):
    """colormap.py:5-85 for a callable of this module: `colormap(disp_err_to_color, est, gt, normalize=False)`.  The string colour
    maps and the min-max normalisation of the reference stay on its side; a batch is coloured whole, not its first image."""
    if not callable(_cmap):
        raise ValueError("only the callables of this module are supported, not the colour map %r" % (_cmap,))
    if normalize:
        raise ValueError("normalize=True is not supported: normalise the input, or use disp_to_color's max_disp")
    return _cmap(*args, format=format, **kwargs)


# ------------------------------------------------------------------------------------------------------------------ optical flow
def make_color_wheel():
    """flow_colormap.py:8-56: the Middlebury colour wheel, float64 [55, 3] with values 0..255: six arcs (red-yellow 15, yellow-green
    6, green-cyan 4, cyan-blue 11, blue-magenta 13, magenta-red 6), on each one channel held at 255 and one ramping by
    floor(255 i / n), up or down."""
    arcs = ((15, 0, 1, True), (6, 1, 0, False), (4, 1, 2, True), (11, 2, 1, False), (13, 2, 0, True), (6, 0, 2, False))
    wheel = np.zeros([sum(a[0] for a in arcs), 3])
    col = 0
    for n, held, ramp, up in arcs:
        step = np.floor(255 * np.arange(0, n) / n)
        wheel[col:col + n, held] = 255
        wheel[col:col + n, ramp] = step if up else 255 - step
        col += n
    return wheel


def _wheel(device):
    key = (device.type, device.index)
    if key not in _WHEEL:
        _WHEEL[key] = torch.from_numpy(make_color_wheel().astype(np.float32)).to(device).contiguous()
    return _WHEEL[key]


def _flow_maps(what, layouts, *tensors):
    """Flow maps of one batch, each [H,W,2] / [B,H,W,2] ('HWC') or [2,H,W] / [B,2,H,W] ('CHW') -> contiguous tensors, B, their
    sizes, and whether a batch axis is returned."""
    _require_gpu(*tensors)
    first = tensors[0]
    out, sizes = [], []
    for t, layout in zip(tensors, layouts):
        if layout not in ('HWC', 'CHW'):
            raise ValueError("layout must be 'HWC' or 'CHW' (got %r)" % (layout,))
        if t is None:
            out.append(None)
            sizes.append(None)
            continue
        if t.dim() not in (3, 4) or t.dim() != first.dim():
            raise ValueError("%s: flow maps must be [H,W,2] / [B,H,W,2] or [2,H,W] / [B,2,H,W], all of one rank (got %s)"
                             % (what, [tuple(x.shape) for x in tensors if x is not None]))
        if t.shape[-1 if layout == 'HWC' else -3] != 2:
            raise ValueError("%s: two channels expected in layout %s, got shape %s" % (what, layout, tuple(t.shape)))
        if t.dim() == 4 and t.shape[0] != first.shape[0]:
            raise ValueError("%s: batch sizes differ (%d and %d)" % (what, first.shape[0], t.shape[0]))
        if t.numel() == 0:
            raise ValueError("%s: empty map of shape %s" % (what, tuple(t.shape)))
        out.append(_lib.contiguous(t))
        sizes.append(tuple(t.shape[-3:-1]) if layout == 'HWC' else tuple(t.shape[-2:]))
    return out, (first.shape[0] if first.dim() == 4 else 1), sizes, first.dim() == 4


def _flow_render(est, gt, val, layouts, hw, B, size, flags, max_rad=None, batched=True, dtype=torch.float32, format='HWC'):
    """One ts_flow_render_fwd call.  Returns {'flow_color', 'err_class', 'stats'}: those that flags selects."""
    dev = est.device
    Hg, Wg = size
    L = _lib.lib()
    res = {}
    flags |= (FLOW_EST_HWC if layouts[0] == 'HWC' else 0) | (FLOW_GT_HWC if gt is not None and layouts[1] == 'HWC' else 0)
    shape = (lambda rows: (B, 3, rows, Wg)) if format == 'CHW' else (lambda rows: (B, rows, Wg, 3))
    colors = flags & (FLOW_EST_COLOR | FLOW_GT_COLOR)
    if colors:
        res['flow_color'] = torch.empty(shape(2 * Hg if colors == FLOW_EST_COLOR | FLOW_GT_COLOR else Hg), device=dev, dtype=dtype)
    if flags & FLOW_ERR_CLASS:
        res['err_class'] = torch.empty(shape(Hg), device=dev, dtype=dtype)
    maxr = None
    if max_rad is not None and colors:
        if torch.is_tensor(max_rad):
            _require_gpu(max_rad)
            if max_rad.numel() != B:
                raise ValueError("max_rad must hold one maximum per image (%d), got shape %s" % (B, tuple(max_rad.shape)))
            maxr = _lib.contiguous(max_rad.reshape(B))
        else:
            maxr = torch.full((B,), float(max_rad), device=dev, dtype=torch.float32)
        flags |= FLOW_MAX_GIVEN
    stats = ws = None
    if flags & FLOW_STATS or (colors and maxr is None):
        stats = torch.empty((B, FLOW_STATS_FLOATS), device=dev, dtype=torch.float32)
        ws = torch.empty(int(L.ts_flow_render_workspace_bytes(B, Hg, Wg)), device=dev, dtype=torch.uint8)
        res['stats'] = stats
    wheel = _wheel(dev) if colors else None
    _lib.check(L.ts_flow_render_fwd(_lib.ptr(est), _lib.ptr(gt), _lib.ptr(val), _lib.ptr(maxr), _lib.ptr(wheel), B, hw[0], hw[1],
                                    Hg, Wg, flags, _lib.ptr(res.get('flow_color')), _lib.ptr(res.get('err_class')), _lib.ptr(stats),
                                    _lib.ptr(ws), _stream()), "ts_flow_render_fwd")
    if not batched:
        res = {k: (v[0] if k != 'stats' else v) for k, v in res.items()}
    return res


def _flow_valid(what, val, B, size, batched):
    """F_gt_val [H,W] / [B,H,W] / [B,1,H,W] as a contiguous fp32 map; a bool or uint8 mask is converted (not while recording)."""
    if val is None:
        return None
    if not torch.is_tensor(val):
        raise TypeError("%s: the validity map must be a tensor, got %s" % (what, type(val).__name__))
    if val.dtype in (torch.bool, torch.uint8) and val.is_cuda:
        if _lib.recording():
            raise RuntimeError("%s: a bool / uint8 validity map needs a cast that a launch plan would not replay; hand over fp32" % what)
        val = val.to(torch.float32)
    _require_gpu(val)
    if val.numel() != B * size[0] * size[1] or tuple(val.shape[-2:]) != tuple(size):
        raise ValueError("%s: a validity map of shape %s for %d maps of size %s" % (what, tuple(val.shape), B, tuple(size)))
    return _lib.contiguous(val)


def flow_max_rad(flow, layout='HWC'):
    """flow_colormap.py:59-77: the maximum of sqrt(u^2 + v^2) with unknown pixels as (0, 0): a 0-dim device tensor, or [B] for a
    batch (one per image).  `flow` is not modified."""
    (f,), B, (hw,), batched = _flow_maps("flow_max_rad", (layout,), flow)
    stats = _flow_render(f, None, None, (layout, layout), hw, B, hw, FLOW_STATS)['stats']
    return stats[:, 0] if batched else stats[0, 0]


def flow_to_color(flow, max_rad=None, layout='HWC', dtype=torch.float32, format='HWC'):
    """flow_colormap.py:143-167: the Middlebury colours of flow ([H,W,2] -> [H,W,3]; [B,H,W,2] -> [B,H,W,3]; layout='CHW': [2,H,W] /
    [B,2,H,W]).  max_rad: None (each image's own maximum radius, found on the device), a number, or a [B] device tensor."""
    (f,), B, (hw,), batched = _flow_maps("flow_to_color", (layout,), flow)
    return _flow_render(f, None, None, (layout, layout), hw, B, hw, FLOW_EST_COLOR | _flow_fmt(dtype, format), max_rad=max_rad,
                        batched=batched, dtype=dtype, format=format)['flow_color']


def flow_color(flow, max_rad=None, layout='HWC', dtype=torch.float32, format='HWC'):
    """flow_colormap.py:80-140: as flow_to_color (the reference's two functions blacken unknown pixels in two ways, with one result)."""
    return flow_to_color(flow, max_rad=max_rad, layout=layout, dtype=dtype, format=format)


def flow_err_to_color(F_est, F_gt, F_gt_val=None, layout='HWC', dtype=torch.float32, format='HWC'):
    """flow_colormap.py:170-220: the KITTI error classes of F_est against F_gt (one shape); F_gt_val ([H,W] / [B,H,W], fp32 or a
    bool / uint8 mask) multiplies the error, and where it is 0 the pixel is black."""
    (e, g), B, (hw, ghw), batched = _flow_maps("flow_err_to_color", (layout, layout), F_est, F_gt)
    if hw != ghw:
        raise ValueError("F_est has shape %s, F_gt %s" % (tuple(F_est.shape), tuple(F_gt.shape)))
    val = _flow_valid("flow_err_to_color", F_gt_val, B, hw, batched)
    return _flow_render(e, g, val, (layout, layout), hw, B, hw, FLOW_ERR_CLASS | _flow_fmt(dtype, format), batched=batched,
                        dtype=dtype, format=format)['err_class']


def _flow_fmt(dtype, format):
    f = _fmt(dtype, format)
    return (FLOW_UINT8 if f & UINT8 else 0) | (FLOW_CHW if f & CHW else 0)


def flow_render_stats(flow, gt=None, valid=None, size=None, layout='CHW'):
    """The per-image statistics of a frame, [B, 16] fp32 on the device (layout: include/ts_hip.h), of flow rescaled to gt's size
    (or `size`): the maximum radius of flow, of gt and of both, and the members' counts of the ten error classes."""
    (e, g), B, (hw, ghw), batched = _flow_maps("flow_render_stats", (layout, layout), flow, gt)
    size = _target(hw, ghw, size)
    return _flow_render(e, g, _flow_valid("flow_render_stats", valid, B, size, batched), (layout, layout), hw, B, size, FLOW_STATS)['stats']


def flow_class_counts(stats):
    """The members' counts of the ten error classes, [B, 10] int32, out of a flow_render_stats tensor."""
    return stats[:, 4:14].contiguous().view(torch.int32)


def render_flow_frame(flow, gt=None, valid=None, size=None, outputs=None, dtype=torch.uint8, format='HWC', layout='CHW'):
    """The pictures of a frame's flow, fused: flow at its NATIVE resolution ([B,2,h,w] or [2,h,w]; layout='HWC': [B,h,w,2] / [h,w,2])
    is read through the align-corners rescale to gt's size (or `size`; u scaled by W / w, v by H / h) and never written at full
    size.  Returns a dict of device tensors, those of `outputs` (default: all that apply):
      'flow_color'   the estimate's flow colours above the ground truth's, one shared maximum radius per image, [B,2H,W,3];
                     without gt the estimate alone with its own maximum, [B,H,W,3]
      'error_map'    flow_err_to_color of the rescaled estimate against gt, `valid` as F_gt_val        needs gt
    One statistics launch pair and one colour launch for the whole dict, batched over B."""
    (e, g), B, (hw, ghw), batched = _flow_maps("render_flow_frame", (layout, layout), flow, gt)
    size = _target(hw, ghw, size)
    if valid is not None and g is None:
        raise ValueError("render_flow_frame: a validity map without a ground truth")
    if outputs is None:
        outputs = FLOW_OUTPUTS if g is not None else ('flow_color',)
    flags = _flow_fmt(dtype, format)
    for o in outputs:
        if o not in FLOW_OUTPUTS:
            raise ValueError("unknown output %r (one of %s)" % (o, FLOW_OUTPUTS))
        if g is None and o == 'error_map':
            raise ValueError("%s needs a ground truth" % o)
        flags |= {'flow_color': FLOW_EST_COLOR | (FLOW_GT_COLOR | FLOW_MAX_SHARED if g is not None else 0), 'error_map': FLOW_ERR_CLASS}[o]
    if not outputs:
        return {}
    val = _flow_valid("render_flow_frame", valid, B, size, batched)
    r = _flow_render(e, g, val, (layout, layout), hw, B, size, flags, batched=batched, dtype=dtype, format=format)
    names = {'flow_color': 'flow_color', 'error_map': 'err_class'}
    return {o: r[names[o]] for o in outputs}
