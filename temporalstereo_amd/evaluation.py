"""Disparity evaluation on the device: n-px error, EPE and the occlusion split, on the kernels of csrc/evaluation.hip.

Drop-ins with the reference's signatures, keys and return shapes:
  calc_error                 architecture/data/evaluation/pixel_error.py:6-71
  do_evaluation              architecture/data/evaluation/eval.py:9-42
  do_occlusion_evaluation    architecture/data/evaluation/eval.py:45-105
and `validation_metrics`, the fused form of what `validation_step` / `test_step` do with the returned disparities
(projects/TemporalStereo/TemporalStereo.py:170-214): the rescale to the ground truth's size (:183) plus `log_metric` (:463-486), for
up to four levels per launch pair, the occlusion mask computed once per ground-truth pixel and shared by every level.

Semantics kept from the reference:
  - valid pixels: gt > lb (when lb is given) and gt < ub (when ub is given), both strict; a NaN gt is never valid, a NaN estimate
    inside the mask leaves the counts alone and makes epe NaN, an infinite one counts in every threshold;
  - {1,2,3,5}px = count(|gt - est| > t) / N * 100 in fp32, epe = mean |gt - est|; all five are 0 when no pixel is valid;
  - the occ / noc split is literal: calc_error(est * m, gt * m) with m = occ or 1 - occ, so a pixel outside the split enters as
    gt' = 0, est' = est * 0 -- masked out when lb >= 0, counted with error 0 (NaN for a non-finite est) when lb is None or negative.
Differences, deliberate:
  - every value is a float32 tensor of shape [1] ON THE DEVICE (a view into one output buffer; `.cpu()` gives the reference's
    value).  Nothing here synchronises with the host;
  - counts are exact integers, where the reference counts in fp32 (`mask.float().sum()`, exact only up to 2^24 pixels); epe is
    summed in fp64 in a fixed order and rounded once, so results are bit-identical from run to run;
  - validation_metrics evaluates the rescale with the arithmetic of `losses.rescale_to_full` (interpolate, then scale by Wg / w),
    which the reference does in the other order (scale, then interpolate): within an ulp of the reference's map, and bit-identical to
    `do_evaluation(rescale_to_full(d, (Hg, Wg)), gt)`.
fp32 GPU tensors only: a CPU tensor raises, there is no CPU fallback.

Optical flow, on the kernels of csrc/flow_frame.hip -- drop-ins with the reference's signatures, keys and return shapes:
  flow_calc_error            architecture/data/evaluation/flow_pixel_error.py:9-96
  do_flow_evaluation         architecture/data/evaluation/flow_eval.py:6-37
and `flow_validation_metrics`, the fused multi-level form: up to four estimates [B,2,h,w] at their native resolutions against one
ground truth per launch pair.
Semantics kept from the reference:
  - valid pixels: no NaN in either ground-truth component, lb < sqrt(gt_u^2 + gt_v^2) < ub (both strict) and, with sparse=True,
    not (|gt_u| < 1e-12 and |gt_v| < 1e-12); err = sqrt((gt_u - est_u)^2 + (gt_v - est_v)^2), both radii in fp32 with every
    operation rounded on its own, so the counts are the reference's;
  - {1,2,3,5}px = count(err > t) / N * 100 in fp32, epe = mean err; all five are 0 when no pixel is valid; a NaN estimate inside the
    mask leaves the counts alone and makes epe NaN;
  - the early returns: CPU zeros when an argument is not a tensor, a warning and {} for a None in do_flow_evaluation;
  - the quirk of do_flow_evaluation: it does NOT pass lb / ub on (flow_eval.py:35), so its bounds are always 0.0 and 400.
Differences, deliberate:
  - values are [1]-shaped fp32 views of one device buffer, counts exact integers, epe summed in fp64 in a fixed order, as above;
  - flow_validation_metrics rescales a smaller or larger estimate with the arithmetic of `losses.rescale_to_full` (align-corners
    bilinear, then u * Wg / w and v * Hg / h).  The reference has no rescale for flow: this one is defined by that torch composition.
"""
import warnings

import torch

from . import _lib
from .functional import _require_gpu, _stream

KEYS = ('1px', '2px', '3px', '5px', 'epe')
SPLITS = ('all', 'occ', 'noc')
MAX_LEVELS = 4          # levels per ts_disp_metrics_fwd / ts_flow_metrics_fwd call
FLOW_SPARSE, FLOW_EST_HWC, FLOW_GT_HWC = 1, 2, 4          # flag word of ts_flow_metrics_fwd (include/ts_hip.h)


def _zero_dict(prefix=''):
    # the reference's early return (pixel_error.py:17-31): CPU zeros, the percentages multiplied by 100
    return {prefix + k: torch.Tensor([0.]) * (100 if k != 'epe' else 1) for k in KEYS}


def _metrics(ests, gt, gt_right, lb, ub):
    """One ts_disp_metrics_fwd call over 1..4 estimates against gt ([..., Hg, Wg]); out [n, 3, 5] (all / occ / noc x KEYS)."""
    _require_gpu(*ests, gt, gt_right)
    if not 1 <= len(ests) <= MAX_LEVELS:
        raise ValueError("between 1 and %d disparities per call (got %d)" % (MAX_LEVELS, len(ests)))
    if gt.dim() < 2:
        raise ValueError("the ground truth must be [..., H, W]")
    Hg, Wg = gt.shape[-2:]
    B = gt.numel() // (Hg * Wg) if Hg * Wg else 0
    dims = []
    for e in ests:
        if e.shape == gt.shape:
            dims.append((Hg, Wg))
        elif e.dim() == 4 and gt.dim() == 4 and e.shape[:2] == gt.shape[:2] and gt.shape[1] == 1:
            dims.append(tuple(e.shape[-2:]))
        else:
            raise ValueError("disparity of shape %s against a ground truth of shape %s" % (tuple(e.shape), tuple(gt.shape)))
    if gt_right is not None:
        if gt_right.shape != gt.shape or gt.dim() != 4 or gt.shape[1] != 1:
            raise ValueError("the left and right ground truths must be [B,1,H,W] of one shape (got %s and %s)"
                             % (tuple(gt.shape), tuple(gt_right.shape)))
        if Hg < 2 or Wg < 2:
            raise ValueError("the occlusion warp needs H, W >= 2 (inverse_warp divides by H-1 and W-1)")
    out_shape = (len(ests), len(SPLITS), len(KEYS))
    if B == 0 or any(h * w == 0 for h, w in dims):
        return torch.zeros(out_shape, device=gt.device, dtype=torch.float32)       # nothing valid: the reference's zeros
    ests = [_lib.contiguous(e) for e in ests]
    gt = _lib.contiguous(gt)
    gt_right = _lib.contiguous(gt_right) if gt_right is not None else None
    L = _lib.lib()
    out = torch.empty(out_shape, device=gt.device, dtype=torch.float32)
    ws = torch.empty(int(L.ts_disp_metrics_workspace_bytes(B, Hg, Wg)), device=gt.device, dtype=torch.uint8)
    p = [_lib.ptr(e) for e in ests] + [None] * (MAX_LEVELS - len(ests))
    hw = [v for d in dims + [(0, 0)] * (MAX_LEVELS - len(dims)) for v in d]
    flags = (1 if lb is not None else 0) | (2 if ub is not None else 0)
    _lib.check(L.ts_disp_metrics_fwd(*p, len(ests), *hw, _lib.ptr(gt), _lib.ptr(gt_right), B, Hg, Wg,
                                     float(lb) if lb is not None else 0.0, float(ub) if ub is not None else 0.0, flags,
                                     _lib.ptr(out), _lib.ptr(ws), _stream()), "ts_disp_metrics_fwd")
    return out


def _as_dict(out, level, split, prefix=''):
    s = SPLITS.index(split)
    return {prefix + k: out[level, s, i:i + 1] for i, k in enumerate(KEYS)}


def calc_error(est_disp=None, gt_disp=None, lb=None, ub=None):
    """pixel_error.py:6-71: {'1px', '2px', '3px', '5px': percent, 'epe'} of est_disp against gt_disp ([..., H, W], one shape)."""
    if not torch.is_tensor(est_disp) or not torch.is_tensor(gt_disp):
        return _zero_dict()
    if est_disp.shape != gt_disp.shape:
        raise ValueError("est_disp has shape %s, gt_disp %s" % (tuple(est_disp.shape), tuple(gt_disp.shape)))
    return _as_dict(_metrics([est_disp], gt_disp, None, lb, ub), 0, 'all')


def do_evaluation(est_disp, gt_disp, lb, ub):
    """eval.py:9-42: calc_error after the reference's None checks (a warning and {})."""
    if est_disp is None:
        warnings.warn('Estimated disparity map is None')
        return {}
    if gt_disp is None:
        warnings.warn('Reference ground truth disparity map is None')
        return {}
    return calc_error(est_disp, gt_disp, lb=lb, ub=ub)


def do_occlusion_evaluation(est_disp, ref_gt_disp, target_gt_disp, lb, ub):
    """eval.py:45-105: {'occ_1px', ..., 'occ_epe', 'noc_1px', ..., 'noc_epe'} of est_disp [B,1,H,W] on the pixels that the right
    ground truth, warped by the left one, marks occluded (|warp - gt| > 1 or |warp| < 1e-6) and on the others."""
    if est_disp is None:
        warnings.warn('Estimated disparity map is None, expected given')
        return {}
    if ref_gt_disp is None:
        warnings.warn('Reference ground truth disparity map is None, expected given')
        return {}
    if target_gt_disp is None:
        warnings.warn('Target ground truth disparity map is None, expected given')
        return {}
    if not all(torch.is_tensor(t) for t in (est_disp, ref_gt_disp, target_gt_disp)):
        return dict(_zero_dict('occ_'), **_zero_dict('noc_'))
    if est_disp.shape != ref_gt_disp.shape or target_gt_disp.shape != ref_gt_disp.shape:
        raise ValueError("{}, {}, {}".format(tuple(est_disp.shape), tuple(ref_gt_disp.shape), tuple(target_gt_disp.shape)))
    out = _metrics([est_disp], ref_gt_disp, target_gt_disp, lb, ub)
    return dict(_as_dict(out, 0, 'occ', 'occ_'), **_as_dict(out, 0, 'noc', 'noc_'))


def validation_metrics(disps, gt_left, gt_right=None, lb=0, ub=192, eval_ids=None):
    """The metric dict of `log_metric` (TemporalStereo.py:463-486) after validation_step's rescale (:183), fused.

    disps: the aggregation's disparities [B,1,h,w] at their NATIVE resolutions (any size; each is read through the align-corners
    rescale to gt_left's size, value-scaled by Wg / w).  gt_left / gt_right: [B,1,Hg,Wg]; gt_right None skips the occ / noc split
    (as log_metric does without a right ground truth).  lb / ub: VAL.LOWERBOUND / VAL.UPPERBOUND.  eval_ids: VAL.EVAL_DISPARITY_IDS
    (default every level), filtered to the levels present (:469).
    Returns {'metric_disparity_{id}/all_1px': ..., ..., 'metric_disparity_{id}/noc_epe': ...}: [1]-shaped fp32 device tensors.
    One launch pair per group of up to four levels."""
    if gt_left is None:
        return {}
    ids = _eval_ids(len(disps), eval_ids)
    splits = SPLITS if gt_right is not None else SPLITS[:1]
    result = {}
    for g in range(0, len(ids), MAX_LEVELS):
        group = ids[g:g + MAX_LEVELS]
        out = _metrics([disps[i] for i in group], gt_left, gt_right, lb, ub)
        for j, i in enumerate(group):
            for s in splits:
                result.update(_as_dict(out, j, s, 'metric_disparity_{}/{}_'.format(i, s)))
    return result


def _eval_ids(n_levels, eval_ids):
    # VAL.EVAL_DISPARITY_IDS, default every level, filtered to the levels present (TemporalStereo.py:468-469)
    return [i for i in (range(n_levels) if eval_ids is None else eval_ids) if i < n_levels]


def metric_keys(n_levels, eval_ids=None, occlusion=True):
    """The keys validation_metrics returns for n_levels disparities, in its order (that of log_metric)."""
    splits = SPLITS if occlusion else SPLITS[:1]
    return ['metric_disparity_{}/{}_{}'.format(i, s, k) for i in _eval_ids(n_levels, eval_ids) for s in splits for k in KEYS]


def _flow_metrics(ests, gt, lb, ub, sparse):
    """One ts_flow_metrics_fwd call over 1..4 estimates [B,2,h,w] / [2,h,w] against gt [B,2,Hg,Wg] / [2,Hg,Wg]; out [n, 5]."""
    _require_gpu(*ests, gt)
    if not 1 <= len(ests) <= MAX_LEVELS:
        raise ValueError("between 1 and %d flow maps per call (got %d)" % (MAX_LEVELS, len(ests)))
    if gt.dim() not in (3, 4):
        raise ValueError("the ground truth must be [2,H,W] or [B,2,H,W] (got %s)" % (tuple(gt.shape),))
    if gt.shape[-3] != 2:
        raise ValueError("flow should have horizontal and vertical dimension, but got {}".format(gt.shape[-3]))
    B = gt.shape[0] if gt.dim() == 4 else 1
    Hg, Wg = gt.shape[-2:]
    dims = []
    for e in ests:
        if e.dim() != gt.dim() or e.shape[:-2] != gt.shape[:-2]:
            raise ValueError("flow of shape %s against a ground truth of shape %s" % (tuple(e.shape), tuple(gt.shape)))
        dims.append(tuple(e.shape[-2:]))
    out_shape = (len(ests), len(KEYS))
    if B * Hg * Wg == 0 or any(h * w == 0 for h, w in dims):
        return torch.zeros(out_shape, device=gt.device, dtype=torch.float32)       # nothing valid: the reference's zeros
    ests = [_lib.contiguous(e) for e in ests]
    gt = _lib.contiguous(gt)
    L = _lib.lib()
    out = torch.empty(out_shape, device=gt.device, dtype=torch.float32)
    ws = torch.empty(int(L.ts_flow_metrics_workspace_bytes(B, Hg, Wg)), device=gt.device, dtype=torch.uint8)
    p = [_lib.ptr(e) for e in ests] + [None] * (MAX_LEVELS - len(ests))
    hw = [v for d in dims + [(0, 0)] * (MAX_LEVELS - len(dims)) for v in d]
    _lib.check(L.ts_flow_metrics_fwd(*p, len(ests), *hw, _lib.ptr(gt), B, Hg, Wg, float(lb), float(ub), FLOW_SPARSE if sparse else 0,
                                     _lib.ptr(out), _lib.ptr(ws), _stream()), "ts_flow_metrics_fwd")
    return out


def flow_calc_error(est_flow=None, gt_flow=None, lb=0.0, ub=400, sparse=False):
    """flow_pixel_error.py:9-96: {'1px', '2px', '3px', '5px': percent, 'epe'} of est_flow against gt_flow ([2,H,W] or [B,2,H,W], one
    shape) over the pixels with lb < |gt| < ub, no NaN in gt and, with sparse, a ground truth that is not (0, 0)."""
    if not torch.is_tensor(est_flow) or not torch.is_tensor(gt_flow):
        return _zero_dict()
    if est_flow.shape != gt_flow.shape:
        raise ValueError("est_flow has shape %s, gt_flow %s" % (tuple(est_flow.shape), tuple(gt_flow.shape)))
    out = _flow_metrics([est_flow], gt_flow, lb, ub, sparse)
    return {k: out[0, i:i + 1] for i, k in enumerate(KEYS)}


def do_flow_evaluation(est_flow, gt_flow, lb=0.0, ub=400, sparse=False):
    """flow_eval.py:6-37: flow_calc_error after the reference's None checks (a warning and {}).  As in the reference, lb and ub are
    accepted and NOT passed on (:35): the bounds are flow_calc_error's defaults, 0.0 and 400, whatever is given here."""
    if est_flow is None:
        warnings.warn('Estimated flow map is None')
        return {}
    if gt_flow is None:
        warnings.warn('Reference ground truth flow map is None')
        return {}
    return flow_calc_error(est_flow, gt_flow, sparse=sparse)


def flow_validation_metrics(flows, gt_flow, lb=0.0, ub=400, sparse=False, eval_ids=None):
    """flow_calc_error of several estimates, fused.  flows: flow maps [B,2,h,w] at their NATIVE resolutions (each is read through the
    align-corners rescale to gt_flow's size, u scaled by Wg / w and v by Hg / h); gt_flow [B,2,Hg,Wg]; eval_ids: the levels to
    score (default every level), filtered to the levels present.
    Returns {'metric_flow_{id}/all_1px': ..., ..., 'metric_flow_{id}/all_epe': ...}: [1]-shaped fp32 device tensors.
    One launch pair per group of up to four levels."""
    if gt_flow is None:
        return {}
    ids = _eval_ids(len(flows), eval_ids)
    result = {}
    for g in range(0, len(ids), MAX_LEVELS):
        group = ids[g:g + MAX_LEVELS]
        out = _flow_metrics([flows[i] for i in group], gt_flow, lb, ub, sparse)
        for j, i in enumerate(group):
            result.update({'metric_flow_{}/all_{}'.format(i, k): out[j, n:n + 1] for n, k in enumerate(KEYS)})
    return result


def flow_metric_keys(n_levels, eval_ids=None):
    """The keys flow_validation_metrics returns for n_levels flow maps, in its order."""
    return ['metric_flow_{}/all_{}'.format(i, k) for i in _eval_ids(n_levels, eval_ids) for k in KEYS]
