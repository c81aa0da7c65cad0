"""Input frames prepared on the device, on the kernels of csrc/preprocess.hip: uint8 frames in, the batch dictionary out.

What the reference does on the host for every frame, restated on device tensors:
  read_image                     projects/TemporalStereo/video_inference.py:100-110   ToTensor, normalize, F.interpolate
  StereoDatasetBase.do_transform architecture/data/datasets/base.py:99-187            the same, "pad by resize" (:183) for evaluation,
                                                                                      a crop window (:155) for training
  StereoDatasetBase.__getitem__  base.py:231-248, video_inference.py:246-251          the ('K', s) / ('inv_K', s) pyramid
  read_disparity                 video_inference.py:135-140                           (raw * (raw > 0)) / 256.0
  the batch dictionary           video_inference.py:262-293                           `prepare_batch`

Semantics kept from the reference:
  - ('color', t, side) is byte / 255; ('color_aug', t, side) is ((byte / 255) - mean[c]) / std[c] in fp32 with correctly rounded
    divisions, in that order, and only THEN resized (bilinear, align_corners=True).  Without a resize every value has the
    reference's bits; a resized value is within the distance the reference's own fp32 run keeps from a float64 run;
  - evaluation form (`size` alone): `color` keeps the source size, `color_aug` is resized, up or down (base.py:183);
    training form (`size` and `crop`): both are the window [ch:ch+H, cw:cw+W] (base.py:155);
  - the intrinsics of scale s multiply rows 0 / 1 of K_norm by kw // 2**s / kh // 2**s, integer division as written; (kh, kw) is
    the final size for evaluation and the UN-cropped resolution for training (base.py:235-238: pass `k_size`);
  - the 16-bit ground truth is raw / 256 where raw > 0, else 0.
Differences, deliberate:
  - inputs are uint8 GPU tensors, HWC (what a decoder hands over) or CHW, one image or a batch, and both eyes go through ONE launch;
    results are device tensors; nothing here synchronises with the host, so a frame can be prepared inside a stream capture;
  - a crop given as Python ints is refused when it leaves the image; given as an int32 device tensor it cannot be inspected
    without a synchronisation and is CLAMPED into the image by the kernel instead;
  - inv_K is the closed-form inverse evaluated in fp64 and rounded once (the reference: np.linalg.pinv): equal after rounding to
    fp32 within one unit in the last place, and exactly 0 where pinv leaves a residue of ~1e-18;
  - `disp_from_uint16` takes torch.uint16 where this torch has it, or int16 storage REINTERPRETED as unsigned (the bits a 16-bit
    PNG reader hands over viewed as int16); an int32 tensor is accepted with its low 16 bits taken (a cast on the device);
    the valid mask comes from the kernel (torch's comparisons do not cover uint16).
  - `decode_kitti_flow` is the arithmetic of load_png (architecture/data/utils/load_flow.py:54-78) on the raw 16-bit channels of a
    KITTI flow PNG: flow = (raw - 2^15) / 64, exact in fp32, both components 0 where the third channel is 0; the file itself is
    decoded elsewhere.
Out of scope, on purpose: decoding files (PIL / cv2), PFM / .flo loaders.  ColorJitter / gamma, the random occlusion patches of
base.py:157-173 and the ground truth cut to a window whose origin lives on the device are in augment.py (`prepare_train_batch`).
Cropping an fp32 ground-truth map is a tensor slice.
uint8 GPU tensors only: a CPU tensor raises, there is no CPU fallback.
"""
import math

import torch

from . import _lib
from ._frameio import _batch_dict, _color_outputs, _frames, _gt_rows, _on_gpu, _three, _u16_map
from .functional import _stream

IMAGENET_MEAN = (0.485, 0.456, 0.406)       # base.py:41
IMAGENET_STD = (0.229, 0.224, 0.225)
CHW = 1                                     # TS_PREPARE_CHW (include/ts_hip.h)


def prepare_frames(left, right=None, size=None, crop=None, mean=IMAGENET_MEAN, std=IMAGENET_STD, layout='HWC', color=True, out=None):
    """ToTensor + normalize + resize / crop of both eyes in one launch.  left / right: uint8 GPU tensors, [H,W,3] / [B,H,W,3]
    (layout 'HWC') or [3,H,W] / [B,3,H,W] ('CHW').  Returns {'color_l', 'color_aug_l'} and, with `right`, {'color_r', 'color_aug_r'}:
    fp32 [B,3,.,.] ([3,.,.] for an unbatched input); `color=False` leaves the plain / 255 images out.
      size=None, crop=None    the values at the source size
      size=(H, W)             evaluation form: color_aug resized (bilinear, align_corners=True), color at the source size
      size=(H, W), crop=...   training form: the window [ch:ch+H, cw:cw+W] of both; crop is one (ch, cw) per image as a list
                              (checked here, uploaded) or an int32 device tensor [B,2] (clamped into the image by the kernel)
      out=                    pre-allocated color_aug tensor(s), `out_l` or `(out_l, out_r)`, fp32 [B,3,H,W] with dense images
                              and any batch stride (the same for both), e.g. slices of a larger buffer: written in place and
                              returned."""
    what = "prepare_frames"
    left, right, B, Hs, Ws, batched = _frames(what, left, right, layout)
    dev = left.device
    mean, std = _three("mean", mean), _three("std", std)
    if size is None:
        if crop is not None:
            raise ValueError("%s: a crop needs the window's size" % what)
        H, W = Hs, Ws
    else:
        H, W = (int(v) for v in size)
        if H <= 0 or W <= 0:
            raise ValueError("%s: size %s" % (what, (H, W)))
    crop_t = None
    if crop is not None:
        if H > Hs or W > Ws:
            raise ValueError("%s: an image of shape %s cannot be cropped to %s" % (what, (Hs, Ws), (H, W)))
        if torch.is_tensor(crop):
            _on_gpu(what, crop)
            if crop.dtype != torch.int32 or tuple(crop.shape) != (B, 2):
                raise ValueError("%s: a crop tensor is int32 [%d,2] (got %s %s)" % (what, B, crop.dtype, tuple(crop.shape)))
            crop_t = _lib.contiguous(crop)
        else:
            rows = [tuple(int(v) for v in c) for c in ([crop] if len(crop) == 2 and not hasattr(crop[0], '__len__') else crop)]
            if len(rows) == 1 and B > 1:
                rows = rows * B
            if len(rows) != B or any(len(r) != 2 for r in rows):
                raise ValueError("%s: one (ch, cw) per image expected (%d), got %s" % (what, B, rows))
            for ch, cw in rows:
                if not (0 <= ch <= Hs - H and 0 <= cw <= Ws - W):
                    raise ValueError("%s: the crop origin %s puts a %s window outside an image of shape %s" % (what, (ch, cw), (H, W), (Hs, Ws)))
            crop_t = torch.tensor(rows, dtype=torch.int32, device=dev)
    resize = crop_t is None and (H, W) != (Hs, Ws)
    Hc, Wc = (Hs, Ws) if resize else (H, W)
    sides = ('l', 'r') if right is not None else ('l',)
    res, aug_stride = _color_outputs(what, sides, B, H, W, (Hc, Wc), out, color, dev)
    _lib.check(_lib.lib().ts_frames_prepare_fwd(
        _lib.ptr(left), _lib.ptr(right), B, Hs, Ws, CHW if layout == 'CHW' else 0, *mean, *std, H, W, _lib.ptr(crop_t),
        _lib.ptr(res.get('color_l')), _lib.ptr(res.get('color_r')), 3 * Hc * Wc,
        _lib.ptr(res['color_aug_l']), _lib.ptr(res.get('color_aug_r')), aug_stride, _stream()), "ts_frames_prepare_fwd")
    if not batched:
        res = {k: v[0] for k, v in res.items()}
    return res


def default_num_scales(size):
    """min(int(log2(W)), int(log2(H))) of base.py:231"""
    H, W = size
    return min(int(math.log2(W)), int(math.log2(H)))


def intrinsics_pyramid(K_norm, size, num_scales=None):
    """base.py:231-248: K_norm, the intrinsics divided by the image's (h, w) -- fp32 or fp64 GPU tensor [4,4] or [B,4,4] -- and
    size = (kh, kw) -> (K, inv_K), fp32 [B,S,4,4] ([S,4,4] for an unbatched K_norm); [:, s] is ('K', s) / ('inv_K', s)."""
    what = "intrinsics_pyramid"
    _on_gpu(what, K_norm)
    if K_norm.dtype not in (torch.float32, torch.float64):
        raise TypeError("%s: K_norm must be fp32 or fp64 (got %s)" % (what, K_norm.dtype))
    if K_norm.dim() not in (2, 3) or tuple(K_norm.shape[-2:]) != (4, 4) or K_norm.numel() == 0:
        raise ValueError("%s: K_norm must be [4,4] or [B,4,4] (got %s)" % (what, tuple(K_norm.shape)))
    kh, kw = (int(v) for v in size)
    S = default_num_scales((kh, kw)) if num_scales is None else int(num_scales)
    if kh <= 0 or kw <= 0 or S <= 0 or (kh >> (S - 1)) == 0 or (kw >> (S - 1)) == 0:
        raise ValueError("%s: %d scales of a %dx%d image" % (what, S, kh, kw))
    batched = K_norm.dim() == 3
    B = K_norm.shape[0] if batched else 1
    kn = _lib.contiguous(K_norm)
    K = torch.empty((B, S, 4, 4), device=kn.device, dtype=torch.float32)
    inv = torch.empty_like(K)
    _lib.check(_lib.lib().ts_intrinsics_pyramid_fwd(_lib.ptr(kn), 1 if kn.dtype == torch.float64 else 0, B, kh, kw, S, _lib.ptr(K),
                                                    _lib.ptr(inv), _stream()), "ts_intrinsics_pyramid_fwd")
    return (K, inv) if batched else (K[0], inv[0])


def disp_from_uint16(raw, scale=256.0, with_valid=False):
    """video_inference.py:135-140: a 16-bit disparity map [H,W] / [B,H,W] / [B,1,H,W] -> fp32 [H,W] / [B,1,H,W] = raw / scale where
    raw > 0 (exact for scale 256), 0 elsewhere; with_valid also returns the mask raw > 0 (bool, same shape).
    raw: torch.uint16; or torch.int16, whose bits are REINTERPRETED as unsigned (-1 is 65535); or torch.int32, whose low 16 bits
    are taken (a cast on the device; not while a launch plan is being recorded)."""
    r, (B, H, W, batched) = _u16_map("disp_from_uint16", raw, scale)
    disp = torch.empty((B, 1, H, W), device=r.device, dtype=torch.float32)
    valid = torch.empty((B, 1, H, W), device=r.device, dtype=torch.uint8) if with_valid else None
    _lib.check(_lib.lib().ts_disp_u16_decode_fwd(_lib.ptr(r), B, H, W, float(scale), _lib.ptr(disp), _lib.ptr(valid), _stream()),
               "ts_disp_u16_decode_fwd")
    if not batched:
        disp = disp[0, 0]
        valid = valid[0, 0] if with_valid else None
    return (disp, valid.view(torch.bool)) if with_valid else disp


def decode_kitti_flow(raw, layout='HWC'):
    """load_flow.py:54-78 (`load_png`, the arithmetic): the three 16-bit channels of a KITTI flow map, [H,W,3] / [B,H,W,3] (layout
    'HWC', what a PNG reader hands over) or [3,H,W] / [B,3,H,W] ('CHW') -> (flow, valid): flow fp32 [2,H,W] / [B,2,H,W] =
    (raw - 2^15) / 64 with both components 0 where the third channel is 0, valid bool [1,H,W] / [B,1,H,W] = third channel != 0.
    raw: torch.uint16, or torch.int16 whose bits are REINTERPRETED as unsigned.  One launch."""
    what = "decode_kitti_flow"
    if layout not in ('HWC', 'CHW'):
        raise ValueError("layout must be 'HWC' or 'CHW' (got %r)" % (layout,))
    if not torch.is_tensor(raw):
        raise TypeError("%s: expected a tensor, got %s" % (what, type(raw).__name__))
    _on_gpu(what, raw)
    if raw.dtype != torch.int16 and raw.dtype != getattr(torch, "uint16", None):
        raise TypeError("%s: raw must be uint16 or int16 (reinterpreted), got %s" % (what, raw.dtype))
    if raw.dim() not in (3, 4) or raw.shape[-1 if layout == 'HWC' else -3] != 3 or raw.numel() == 0:
        raise ValueError("%s: raw must be a non-empty [H,W,3] / [B,H,W,3] (HWC) or [3,H,W] / [B,3,H,W] (CHW) map, got %s"
                         % (what, tuple(raw.shape)))
    batched = raw.dim() == 4
    B = raw.shape[0] if batched else 1
    H, W = (raw.shape[-3], raw.shape[-2]) if layout == 'HWC' else (raw.shape[-2], raw.shape[-1])
    r = _lib.contiguous(raw)
    flow = torch.empty((B, 2, H, W), device=r.device, dtype=torch.float32)
    valid = torch.empty((B, 1, H, W), device=r.device, dtype=torch.uint8)
    _lib.check(_lib.lib().ts_flow_u16_decode_fwd(_lib.ptr(r), B, H, W, CHW if layout == 'CHW' else 0, _lib.ptr(flow), _lib.ptr(valid),
                                                 _stream()), "ts_flow_u16_decode_fwd")
    valid = valid.view(torch.bool)
    return (flow, valid) if batched else (flow[0], valid[0])


def prepare_batch(left, right, K_norm, baseline, size, timestamp=0, disp_gt_raw=None, crop=None, k_size=None, num_scales=None,
                  mean=IMAGENET_MEAN, std=IMAGENET_STD, layout='HWC', gt_scale=256.0, out=None):
    """The reference's batch dictionary (video_inference.py:262-293; base.py __getitem__) from uint8 frames, in three launches and
    without touching the host:
      ('color', t, 'l' / 'r')       [B,3,Hc,Wc]   ('color_aug', t, 'l' / 'r')  [B,3,H,W]      prepare_frames(size, crop)
      ('K', s), ('inv_K', s)        [B,4,4]       views of the [B,S,4,4] pyramid (batch stride 16 S) for s < num_scales, built at
                                                  k_size (default: `size`; training passes the un-cropped resolution, base.py:235)
      'baseline'                    [B,1,1,1]     a number, or a device tensor of B values
      ('disp_gt', t, 'l')           [B,1,Hg,Wg]   disp_from_uint16(disp_gt_raw, gt_scale) when given
    t = timestamp.  num_scales: None = base.py:231's min(int(log2 W), int(log2 H)) of `size`; video_inference.py uses 1."""
    what = "prepare_batch"
    if right is None:
        raise ValueError("%s: a stereo pair is needed" % what)
    if size is None:
        raise ValueError("%s: the network's input size is needed" % what)
    size = tuple(int(v) for v in size)
    fr = prepare_frames(left, right, size=size, crop=crop, mean=mean, std=std, layout=layout, color=True, out=out)
    S = default_num_scales(size) if num_scales is None else int(num_scales)
    batch = _batch_dict(what, fr, K_norm, size if k_size is None else k_size, S, baseline, timestamp)
    if disp_gt_raw is not None:
        batch[('disp_gt', timestamp, 'l')] = disp_from_uint16(_gt_rows(what, disp_gt_raw, batch), gt_scale)
    return batch
