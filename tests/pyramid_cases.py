"""Test infrastructure: the cases of tests/test_pyramid_ops_gpu.py -- shapes, layouts, contents -- with the error metric, the fp32
yardstick and the bounds, shared with tests/test_pyramid_ref_cpu.py (which pins the yardstick figures written below).  No GPU in here.

Shapes.  The smallest at which each path of csrc/pyramid_ops.hip can still go wrong: the pooling's depth ring in warm-up and tail
(D < 5, D = 5, 6), tiles at and one past PT_Y x PT_X = 8 x 32, H or W < 5; both sides of every DM switch of the merge (8 | 14 | 20);
size-1 axes on either side of a resize; the upsamplers at non-integer ratios.

Metric (that of tests/bn_cases.py).  max |got - ref| per (b, c) plane / that plane's max |ref|, the worst plane counting (`err_planes`);
per tensor for 2-D maps and for gradients (`err_tensor`).  The two softmax upsamplers keep the allclose form of their existing direct
test, tests/test_upsamplers_autograd_gpu.py: max |got - ref| / (atol + rtol |ref|) with that test's rtol / atol, so 1.0 is its bound
(`err_tol`).  Everything that is a move or a comparison (max, sorted samples, gathered columns, all of the merge's backward) has no
bound: it is compared bit for bit.

Bounds.  max(base, 4 x yardstick).  The yardstick of a case is the error, in the same metric, of tests/pyramid_ref.py run on float32
inputs in float32 arithmetic against its float64 run: what the formula itself costs in fp32, never a figure of the kernel under test.
The factor 4 leaves room for summation order (125-term sums, atomics), FMA contraction and the ~1.5 ulp fast SiLU.  Base: the bound
of the op's existing direct test where there is one (1e-5 resize forward and avg, tests/test_native_gpu.py; 1.0 in the upsamplers'
allclose units), else 5e-6 outputs / 2e-5 gradients as bn_cases.BASE.  YARD holds the measured yardsticks; `python tests/pyramid_cases.py`
prints the table.
"""
import collections

import numpy as np
import torch

import pyramid_ref as R
import synth
from sentinel import GUARD, SENTINEL      # noqa: F401

TINY = 1e-30
BASE = {"out": 5e-6, "grad": 2e-5, "avg": 1e-5, "resize": 1e-5, "tol": 1.0}
TS_OK, TS_ERR_SHAPE, TS_ERR_UNSUPPORTED = 0, -2, -3


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _x(shape):
    return "x".join(str(s) for s in shape)


# ---- metric ----------------------------------------------------------------------------------------------------------------------
def err_planes(got, ref):
    """worst (b, c) plane of [B, C, ...]"""
    d = (got.double().cpu() - ref.double()).abs().flatten(2).amax(2)
    return float((d / ref.double().abs().flatten(2).amax(2).clamp_min(TINY)).max())


def err_tensor(got, ref):
    return float((got.double().cpu() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(TINY))


def err_tol(got, ref, rtol, atol):
    ref = ref.double()
    return float(((got.double().cpu() - ref).abs() / (atol + rtol * ref.abs())).max())


def bound(name, quantity, base):
    return max(base, 4.0 * YARD[name][quantity])


# ---- 5^3 pooling -----------------------------------------------------------------------------------------------------------------
POOL_SHAPES = [(1, 1, 1, 1, 1), (1, 2, 2, 3, 4), (2, 3, 4, 5, 6), (1, 2, 5, 8, 32), (1, 2, 6, 9, 33), (2, 3, 7, 17, 70), (1, 1, 12, 4, 40)]
POOL_FWD_CONTENTS = ("n01", "neg", "offset", "quant")
POOL_BWD_CONTENTS = ("n01", "quant", "const", "neg")
POOL_GRADS = ("both", "avg_only", "max_only")          # random grad_avg and grad_max; grad_max zero; grad_avg zero
PoolCase = collections.namedtuple("PoolCase", "name key shape content layout")
POOL_FWD = [PoolCase("pool_%s_%s_%s" % (_x(s), c, L), "pool_%s_%s" % (_x(s), c), s, c, L)
            for s in POOL_SHAPES for c in POOL_FWD_CONTENTS for L in ("dense", "engine")]
POOL_BWD = [PoolCase("poolbwd_%s_%s" % (_x(s), c), "poolbwd_%s_%s" % (_x(s), c), s, c, "dense") for s in POOL_SHAPES for c in POOL_BWD_CONTENTS]


def pool_input(shape, content):
    n = synth.normal(2100 + POOL_SHAPES.index(shape), "x" + content, shape)
    if content == "neg":
        return _t(-np.abs(n) - np.float32(0.5))
    if content == "offset":
        return _t(np.float32(1000.0) + n)
    if content == "quant":
        return _t(np.round(2.0 * n) / 2.0)
    if content == "const":
        return torch.full(shape, 1.5)
    return _t(n)


def pool_grads(shape, which):
    seed = 2200 + POOL_SHAPES.index(shape)
    ga, gm = _t(synth.normal(seed, "ga", shape)), _t(synth.normal(seed, "gm", shape))
    return (torch.zeros(shape) if which == "max_only" else ga), (torch.zeros(shape) if which == "avg_only" else gm)


def measure_pool(case):
    x = pool_input(case.shape, case.content)
    if case in POOL_FWD:
        return {"avg": err_planes(R.pool5(x)[0], R.pool5(x.double())[0])}
    return {w: err_tensor(R.pool5_bwd(x, *pool_grads(case.shape, w)), R.pool5_bwd(x.double(), *[g.double() for g in pool_grads(case.shape, w)]))
            for w in POOL_GRADS}


# ---- merge candidates ------------------------------------------------------------------------------------------------------------
MERGE_K = {1: 0, 8: 3, 9: 4, 14: 5, 15: 6, 20: 8}          # memory candidates of the K > 0 forms per DT = D0 + K
MERGE_HW = [(3, 5), (9, 31)]
MERGE_FORMS = ("e0", "i0", "em", "en", "im")    # explicit | implicit samples x (K = 0 | K > 0 with memory | K > 0 with NULL memory)
MergeCase = collections.namedtuple("MergeCase", "name key DT C hw form layout")
MERGE_FWD = [MergeCase("merge_dt%d_c%d_%dx%d_%s_%s" % (dt, C, hw[0], hw[1], f, L), "merge_dt%d_c%d_%dx%d_%s" % (dt, C, hw[0], hw[1], f), dt, C, hw, f, L)
             for dt in MERGE_K for C in (1, 3, 5) for hw in MERGE_HW for f in MERGE_FORMS if f[1] == "0" or MERGE_K[dt] > 0
             for L in ("dense", "strided")]
MERGE_BWD = [MergeCase("mergebwd_dt%d_c%d_%dx%d" % (dt, C, hw[0], hw[1]), None, dt, C, hw, "em" if MERGE_K[dt] else "e0", "dense")
             for dt in MERGE_K for C in (1, 3, 5) for hw in MERGE_HW]
MERGE_B = 2


def merge_input(case):
    """dict vol, sample, mem_sample, mem_cost, w, scale, shift, D0, K.  Computed samples uniform (0.5, 20) in no order; ties: in
    the pixels px % 3 == 0 the first memory sample equals a computed one (K = 0: the last computed equals the first), in px % 3 == 1
    the last memory sample equals the first, in px % 5 == 2 a 0.0 stands in front of a -0.0 (both below every other sample)."""
    B, C, (H, W), DT = MERGE_B, case.C, case.hw, case.DT
    K = 0 if case.form[1] == "0" else MERGE_K[DT]
    D0 = DT - K
    seed = 2300 + DT * 10 + C
    tag = "%dx%d%s" % (H, W, case.form)
    px = torch.arange(H * W).view(1, H, W).expand(B, H, W)
    d = {"D0": D0, "K": K, "vol": _t(synth.normal(seed, "v" + tag, (B, C, D0, H, W))), "sample": None, "mem_sample": None, "mem_cost": None,
         "w": None, "scale": None, "shift": None}
    implicit = case.form[0] == "i"
    s = torch.arange(D0, dtype=torch.float32).view(1, D0, 1, 1).expand(B, D0, H, W).clone() if implicit else _t(synth.uniform(seed, "s" + tag, (B, D0, H, W), 0.5, 20.0))
    if K > 0:
        d["w"], d["scale"] = _t(synth.normal(seed, "w" + tag, (C,))), _t(synth.uniform(seed, "sc" + tag, (C,), 0.5, 1.5))
        d["shift"] = _t(synth.normal(seed, "sh" + tag, (C,), 0.5))
    if case.form[1] == "m":
        ms = _t(synth.uniform(seed, "ms" + tag, (B, K, H, W), 0.5, 20.0))
        ms[:, 0] = torch.where(px % 3 == 0, s[:, min(1, D0 - 1)], ms[:, 0])
        if K > 1:
            ms[:, K - 1] = torch.where(px % 3 == 1, ms[:, 0], ms[:, K - 1])
        if implicit:                                # candidate 0 IS 0.0: the -0.0 goes into the memory
            ms[:, K // 2] = torch.where(px % 5 == 2, torch.tensor(-0.0), ms[:, K // 2])
        d["mem_sample"], d["mem_cost"] = ms, _t(synth.normal(seed, "mc" + tag, (B, K, H, W), 2.0))
    if not implicit:
        if K == 0 and D0 > 1:
            s[:, D0 - 1] = torch.where(px % 3 == 0, s[:, 0], s[:, D0 - 1])
        if D0 > 1:
            s[:, 0] = torch.where(px % 5 == 2, torch.tensor(0.0), s[:, 0])
            s[:, 1] = torch.where(px % 5 == 2, torch.tensor(-0.0), s[:, 1])
        d["sample"] = s
    return d


def merge_reference(d, dtype=torch.float64):
    c = lambda t: None if t is None else t.to(dtype)
    return R.merge(c(d["vol"]), c(d["sample"]), c(d["mem_sample"]), c(d["mem_cost"]), c(d["w"]), c(d["scale"]), c(d["shift"]), d["K"])


def merge_cat_sample(d):
    """the [B, DT, H, W] candidates in front of the sort (what ts_merge_candidates_bwd is given)"""
    B, _, D0, H, W = d["vol"].shape
    s = d["sample"] if d["sample"] is not None else torch.arange(D0, dtype=torch.float32).view(1, D0, 1, 1).expand(B, D0, H, W)
    return s if d["K"] == 0 else torch.cat([s, d["mem_sample"] if d["mem_sample"] is not None else torch.zeros(B, d["K"], H, W)], 1)


def measure_merge(case):
    """the memory columns are the only arithmetic of this op"""
    d = merge_input(case)
    if d["K"] == 0:
        return {"vol": 0.0}
    return {"vol": err_planes(merge_reference(d, torch.float32)[1], merge_reference(d)[1])}


# ---- trilinear resize + add + act ------------------------------------------------------------------------------------------------
R3_SHAPES = [((3, 5, 7), (3, 5, 7)), ((2, 5, 7), (4, 9, 13)), ((3, 9, 15), (5, 17, 30)), ((1, 1, 1), (3, 4, 5)), ((3, 4, 5), (1, 1, 1)),
             ((4, 6, 8), (1, 6, 1)), ((5, 9, 13), (3, 5, 7))]
R3_BIG = ((3, 100, 150), (6, 200, 300))                    # 360 000 > 1024 x 256 elements per plane set: the grid-stride path
R3Case = collections.namedtuple("R3Case", "name key src dst B C act add layout")     # bwd: add in ("add+g", "add", "none")
R3_FWD = [R3Case("resize_%s_to_%s_a%d_%s_%s" % (_x(s), _x(t), act, add, L), "resize_%s_to_%s_a%d_%s" % (_x(s), _x(t), act, add), s, t, 2, 3, act, add, L)
          for s, t in R3_SHAPES for act in (0, 1) for add in ("add", "noadd") for L in ("dense", "sliced")]
R3_FWD.append(R3Case("resize_%s_to_%s_a1_add_dense" % (_x(R3_BIG[0]), _x(R3_BIG[1])), "resize_%s_to_%s_a1_add" % (_x(R3_BIG[0]), _x(R3_BIG[1])),
                     R3_BIG[0], R3_BIG[1], 1, 1, 1, "add", "dense"))
R3_BWD = [R3Case("resizebwd_%s_to_%s_a%d_%s" % (_x(s), _x(t), act, add), "resizebwd_%s_to_%s_a%d_%s" % (_x(s), _x(t), act, add), s, t, 2, 3, act, add, "dense")
          for s, t in R3_SHAPES for act in (0, 1) for add in ("add+g", "add", "none")]


def r3_input(case):
    seed = 2400 + (R3_SHAPES + [R3_BIG]).index((case.src, case.dst))
    a = _t(synth.normal(seed, "a", (case.B, case.C) + case.src))
    add = _t(synth.normal(seed, "add", (case.B, case.C) + case.dst)) if case.add != "noadd" and case.add != "none" else None
    g = _t(synth.normal(seed, "g", (case.B, case.C) + case.dst))
    return a, add, g


def measure_r3(case):
    a, add, g = r3_input(case)
    dbl = lambda t: None if t is None else t.double()
    if case in R3_FWD:
        return {"out": err_planes(R.resize3d_add_act(a, add, case.dst, case.act), R.resize3d_add_act(a.double(), dbl(add), case.dst, case.act))}
    ga, gb = R.resize3d_add_act_bwd(a, add, g, case.dst, case.act)
    ra, rb = R.resize3d_add_act_bwd(a.double(), dbl(add), g.double(), case.dst, case.act)
    return {"grad_a": err_tensor(ga, ra), "grad_add": err_tensor(gb, rb)}


# ---- bilinear resize, range candidates -------------------------------------------------------------------------------------------
BIL_SHAPES = [((17, 30), (8, 15)), ((5, 7), (5, 7)), ((1, 5), (4, 9)), ((5, 1), (4, 3)), ((4, 6), (1, 1)), ((6, 9), (13, 20))]
BilCase = collections.namedtuple("BilCase", "name key src dst vs layout")
BIL = [BilCase("bilinear_%s_to_%s_s%g_%s" % (_x(s), _x(t), vs, L), "bilinear_%s_to_%s_s%g" % (_x(s), _x(t), vs), s, t, vs, L)
       for s, t in BIL_SHAPES for vs in (1.0, 2.5) for L in ("dense", "padded")]
BIL_PAIR = [BilCase("bilinear_pair_%s_to_%s" % (_x(s), _x(t)), "bilinear_pair_%s_to_%s" % (_x(s), _x(t)), s, t, (1.0, 2.5), "dense") for s, t in BIL_SHAPES]
BIL_B, BIL_C = 2, 3


def bil_input(src, tag="x"):
    return _t(synth.normal(2500 + [s for s, _ in BIL_SHAPES].index(src), tag, (BIL_B, BIL_C) + src, 3.0))


def measure_bil(case):
    x = bil_input(case.src)
    return {"out": err_tensor(R.resize_bilinear(x, case.dst, case.vs), R.resize_bilinear(x.double(), case.dst, case.vs))}


def bil_pair_input(case):
    return bil_input(case.src), bil_input(case.src, "second")


def measure_bil_pair(case):
    return {"map%d" % i: err_tensor(R.resize_bilinear(x, case.dst, vs), R.resize_bilinear(x.double(), case.dst, vs))
            for i, (x, vs) in enumerate(zip(bil_pair_input(case), case.vs))}


RangeCase = collections.namedtuple("RangeCase", "name key hw range coff ctot")
RANGE = [RangeCase("range_%dx%d_r%g_c%d_of%d" % (hw[0], hw[1], r, co, ct), "range_%dx%d_r%g" % (hw[0], hw[1], r), hw, r, co, ct)
         for hw in ((5, 7), (9, 31)) for r in (4.0, 0.0, -2.0) for co, ct in ((0, 5), (2, 8))]
RANGE_B = 2


def range_input(case):
    return _t(synth.uniform(2600, "d%dx%d" % case.hw, (RANGE_B,) + case.hw, 0.0, 48.0))


def measure_range(case):
    d = range_input(case)
    r32, r64 = R.range_candidates(d, case.range), R.range_candidates(d.double(), case.range)
    return {q: err_tensor(a, b) for q, a, b in zip(("low", "high", "cand"), r32, r64)}


# ---- the two softmax upsamplers --------------------------------------------------------------------------------------------------
UpCase = collections.namedtuple("UpCase", "name key kind dims logit_scale")
UNET_DIMS = [(5, 7, 15, 24), (6, 9, 12, 20), (4, 8, 4, 8), (4, 8, 12, 24), (1, 5, 4, 20), (5, 1, 20, 4), (3, 5, 7, 10)]      # (h, w, Ho, Wo)
CONVEX_DIMS = [(1, 6, 2), (5, 1, 2), (4, 5, 1), (3, 4, 3)]                                                                  # (H, W, r)
UPS = [UpCase("%s_%s_x%d" % (kind, _x(d), ls), "%s_%s_x%d" % (kind, _x(d), ls), kind, d, ls)
       for kind, dims in (("unet", UNET_DIMS), ("convex", CONVEX_DIMS)) for d in dims for ls in (1, 30)]
UP_B = 2
# (rtol, atol) of out, grad_logits, grad_disp in tests/test_upsamplers_autograd_gpu.py
UP_TOL = {"convex": ((1e-5, 1e-5), (1e-4, 1e-5), (1e-4, 1e-5)), "unet": ((2e-5, 2e-4), (1e-4, 2e-3), (1e-4, 1e-4))}
UP_QUANTITIES = ("out", "grad_logits", "grad_disp")


def up_input(case):
    """logits (N(0, 2) times the case's scale), disp, grad_out as in the existing direct test"""
    if case.kind == "unet":
        h, w, Ho, Wo = case.dims
        seed = 2700 + UNET_DIMS.index(case.dims)
        return (_t(synth.normal(seed, "m", (UP_B, 9, Ho, Wo), 2.0)) * case.logit_scale, _t(synth.uniform(seed, "d", (UP_B, 1, h, w), 0.0, 40.0)),
                _t(synth.normal(seed, "g", (UP_B, 1, Ho, Wo))))
    H, W, r = case.dims
    seed = 2800 + CONVEX_DIMS.index(case.dims)
    return (_t(synth.normal(seed, "m", (UP_B, 9 * r * r, H, W), 2.0)) * case.logit_scale, _t(synth.uniform(seed, "d", (UP_B, 1, H, W), 0.0, 30.0)),
            _t(synth.normal(seed, "g", (UP_B, 1, H * r, W * r))))


def up_reference(case, dtype=torch.float64):
    """-> (out, grad_logits, grad_disp) of the reference's formulation in `dtype`"""
    logits, disp, g = [t.to(dtype) for t in up_input(case)]
    logits.requires_grad_(True)
    disp.requires_grad_(True)
    out = R.unet_upsample(logits, disp) if case.kind == "unet" else R.convex_upsample(logits, disp, case.dims[2], float(case.dims[2]))
    out.backward(g)
    return out.detach(), logits.grad, disp.grad


def measure_up(case):
    r32, r64 = up_reference(case, torch.float32), up_reference(case)
    return {q: err_tol(a, b, *tol) for q, a, b, tol in zip(UP_QUANTITIES, r32, r64, UP_TOL[case.kind])}


# ---- the yardstick table ---------------------------------------------------------------------------------------------------------
def measured():
    """every (key, measuring function, case) that has a yardstick: one per distinct input (the layouts of a case share theirs)"""
    seen = {}
    for cases, fn in ((POOL_FWD, measure_pool), (POOL_BWD, measure_pool), (MERGE_FWD, measure_merge), (R3_FWD, measure_r3), (R3_BWD, measure_r3),
                      (BIL, measure_bil), (BIL_PAIR, measure_bil_pair), (RANGE, measure_range), (UPS, measure_up)):
        for c in cases:
            seen.setdefault(c.key, (fn, c))
    return seen


# key: {quantity: error of the float32 evaluation of pyramid_ref against its float64 evaluation, in the quantity's metric}
YARD = {
    "pool_1x1x1x1x1_n01": {"avg": 2.33e-08},
    "pool_1x1x1x1x1_neg": {"avg": 4.06e-08},
    "pool_1x1x1x1x1_offset": {"avg": 4.67e-08},
    "pool_1x1x1x1x1_quant": {"avg": 4.75e-08},
    "pool_1x2x2x3x4_n01": {"avg": 2.44e-07},
    "pool_1x2x2x3x4_neg": {"avg": 1.3e-07},
    "pool_1x2x2x3x4_offset": {"avg": 1.28e-07},
    "pool_1x2x2x3x4_quant": {"avg": 2.24e-08},
    "pool_2x3x4x5x6_n01": {"avg": 1.83e-07},
    "pool_2x3x4x5x6_neg": {"avg": 1.48e-07},
    "pool_2x3x4x5x6_offset": {"avg": 1.25e-07},
    "pool_2x3x4x5x6_quant": {"avg": 4.75e-08},
    "pool_1x2x5x8x32_n01": {"avg": 1.19e-07},
    "pool_1x2x5x8x32_neg": {"avg": 1.78e-07},
    "pool_1x2x5x8x32_offset": {"avg": 1.4e-07},
    "pool_1x2x5x8x32_quant": {"avg": 3.42e-08},
    "pool_1x2x6x9x33_n01": {"avg": 1.36e-07},
    "pool_1x2x6x9x33_neg": {"avg": 2.26e-07},
    "pool_1x2x6x9x33_offset": {"avg": 1.48e-07},
    "pool_1x2x6x9x33_quant": {"avg": 4.6e-08},
    "pool_2x3x7x17x70_n01": {"avg": 1.53e-07},
    "pool_2x3x7x17x70_neg": {"avg": 2.01e-07},
    "pool_2x3x7x17x70_offset": {"avg": 1.65e-07},
    "pool_2x3x7x17x70_quant": {"avg": 4.86e-08},
    "pool_1x1x12x4x40_n01": {"avg": 1.13e-07},
    "pool_1x1x12x4x40_neg": {"avg": 1.7e-07},
    "pool_1x1x12x4x40_offset": {"avg": 1.69e-07},
    "pool_1x1x12x4x40_quant": {"avg": 3.24e-08},
    "poolbwd_1x1x1x1x1_n01": {"both": 2.32e-08, "avg_only": 1.99e-08, "max_only": 0},
    "poolbwd_1x1x1x1x1_quant": {"both": 2.32e-08, "avg_only": 1.99e-08, "max_only": 0},
    "poolbwd_1x1x1x1x1_const": {"both": 2.32e-08, "avg_only": 1.99e-08, "max_only": 0},
    "poolbwd_1x1x1x1x1_neg": {"both": 2.32e-08, "avg_only": 1.99e-08, "max_only": 0},
    "poolbwd_1x2x2x3x4_n01": {"both": 4.59e-08, "avg_only": 1.6e-07, "max_only": 1.3e-07},
    "poolbwd_1x2x2x3x4_quant": {"both": 8.92e-08, "avg_only": 1.6e-07, "max_only": 6.37e-08},
    "poolbwd_1x2x2x3x4_const": {"both": 8.92e-08, "avg_only": 1.6e-07, "max_only": 8.81e-08},
    "poolbwd_1x2x2x3x4_neg": {"both": 4.59e-08, "avg_only": 1.6e-07, "max_only": 1.3e-07},
    "poolbwd_2x3x4x5x6_n01": {"both": 1.82e-07, "avg_only": 1.52e-07, "max_only": 1.97e-07},
    "poolbwd_2x3x4x5x6_quant": {"both": 2.35e-07, "avg_only": 1.52e-07, "max_only": 1.84e-07},
    "poolbwd_2x3x4x5x6_const": {"both": 1.28e-07, "avg_only": 1.52e-07, "max_only": 7.59e-08},
    "poolbwd_2x3x4x5x6_neg": {"both": 1.95e-07, "avg_only": 1.52e-07, "max_only": 1.82e-07},
    "poolbwd_1x2x5x8x32_n01": {"both": 1.79e-07, "avg_only": 1.13e-07, "max_only": 1.68e-07},
    "poolbwd_1x2x5x8x32_quant": {"both": 1.81e-07, "avg_only": 1.13e-07, "max_only": 1.87e-07},
    "poolbwd_1x2x5x8x32_const": {"both": 4.94e-08, "avg_only": 1.13e-07, "max_only": 7.69e-08},
    "poolbwd_1x2x5x8x32_neg": {"both": 1.06e-07, "avg_only": 1.13e-07, "max_only": 1.61e-07},
    "poolbwd_1x2x6x9x33_n01": {"both": 2.08e-07, "avg_only": 1.26e-07, "max_only": 2.75e-07},
    "poolbwd_1x2x6x9x33_quant": {"both": 1.87e-07, "avg_only": 1.26e-07, "max_only": 1.68e-07},
    "poolbwd_1x2x6x9x33_const": {"both": 6.84e-08, "avg_only": 1.26e-07, "max_only": 9.68e-08},
    "poolbwd_1x2x6x9x33_neg": {"both": 9.71e-08, "avg_only": 1.26e-07, "max_only": 1.33e-07},
    "poolbwd_2x3x7x17x70_n01": {"both": 1.56e-07, "avg_only": 1.21e-07, "max_only": 1.81e-07},
    "poolbwd_2x3x7x17x70_quant": {"both": 2.85e-07, "avg_only": 1.21e-07, "max_only": 2.83e-07},
    "poolbwd_2x3x7x17x70_const": {"both": 1.04e-07, "avg_only": 1.21e-07, "max_only": 8.56e-08},
    "poolbwd_2x3x7x17x70_neg": {"both": 3.37e-07, "avg_only": 1.21e-07, "max_only": 2.76e-07},
    "poolbwd_1x1x12x4x40_n01": {"both": 1.27e-07, "avg_only": 1.37e-07, "max_only": 2.15e-07},
    "poolbwd_1x1x12x4x40_quant": {"both": 1.42e-07, "avg_only": 1.37e-07, "max_only": 1.22e-07},
    "poolbwd_1x1x12x4x40_const": {"both": 9.1e-08, "avg_only": 1.37e-07, "max_only": 4.99e-08},
    "poolbwd_1x1x12x4x40_neg": {"both": 2.43e-07, "avg_only": 1.37e-07, "max_only": 3.11e-07},
    "merge_dt1_c1_3x5_e0": {"vol": 0},
    "merge_dt1_c1_3x5_i0": {"vol": 0},
    "merge_dt1_c1_9x31_e0": {"vol": 0},
    "merge_dt1_c1_9x31_i0": {"vol": 0},
    "merge_dt1_c3_3x5_e0": {"vol": 0},
    "merge_dt1_c3_3x5_i0": {"vol": 0},
    "merge_dt1_c3_9x31_e0": {"vol": 0},
    "merge_dt1_c3_9x31_i0": {"vol": 0},
    "merge_dt1_c5_3x5_e0": {"vol": 0},
    "merge_dt1_c5_3x5_i0": {"vol": 0},
    "merge_dt1_c5_9x31_e0": {"vol": 0},
    "merge_dt1_c5_9x31_i0": {"vol": 0},
    "merge_dt8_c1_3x5_e0": {"vol": 0},
    "merge_dt8_c1_3x5_i0": {"vol": 0},
    "merge_dt8_c1_3x5_em": {"vol": 1.02e-07},
    "merge_dt8_c1_3x5_en": {"vol": 3.28e-09},
    "merge_dt8_c1_3x5_im": {"vol": 6.38e-08},
    "merge_dt8_c1_9x31_e0": {"vol": 0},
    "merge_dt8_c1_9x31_i0": {"vol": 0},
    "merge_dt8_c1_9x31_em": {"vol": 2.21e-08},
    "merge_dt8_c1_9x31_en": {"vol": 1.32e-10},
    "merge_dt8_c1_9x31_im": {"vol": 1.25e-07},
    "merge_dt8_c3_3x5_e0": {"vol": 0},
    "merge_dt8_c3_3x5_i0": {"vol": 0},
    "merge_dt8_c3_3x5_em": {"vol": 1.16e-07},
    "merge_dt8_c3_3x5_en": {"vol": 2.21e-09},
    "merge_dt8_c3_3x5_im": {"vol": 2.11e-07},
    "merge_dt8_c3_9x31_e0": {"vol": 0},
    "merge_dt8_c3_9x31_i0": {"vol": 0},
    "merge_dt8_c3_9x31_em": {"vol": 1.29e-07},
    "merge_dt8_c3_9x31_en": {"vol": 7.83e-09},
    "merge_dt8_c3_9x31_im": {"vol": 1.02e-07},
    "merge_dt8_c5_3x5_e0": {"vol": 0},
    "merge_dt8_c5_3x5_i0": {"vol": 0},
    "merge_dt8_c5_3x5_em": {"vol": 1.01e-07},
    "merge_dt8_c5_3x5_en": {"vol": 6.98e-09},
    "merge_dt8_c5_3x5_im": {"vol": 1.44e-07},
    "merge_dt8_c5_9x31_e0": {"vol": 0},
    "merge_dt8_c5_9x31_i0": {"vol": 0},
    "merge_dt8_c5_9x31_em": {"vol": 1.55e-07},
    "merge_dt8_c5_9x31_en": {"vol": 3.83e-09},
    "merge_dt8_c5_9x31_im": {"vol": 1.36e-07},
    "merge_dt9_c1_3x5_e0": {"vol": 0},
    "merge_dt9_c1_3x5_i0": {"vol": 0},
    "merge_dt9_c1_3x5_em": {"vol": 1.07e-08},
    "merge_dt9_c1_3x5_en": {"vol": 1.56e-09},
    "merge_dt9_c1_3x5_im": {"vol": 8.26e-08},
    "merge_dt9_c1_9x31_e0": {"vol": 0},
    "merge_dt9_c1_9x31_i0": {"vol": 0},
    "merge_dt9_c1_9x31_em": {"vol": 3.82e-08},
    "merge_dt9_c1_9x31_en": {"vol": 5.41e-09},
    "merge_dt9_c1_9x31_im": {"vol": 1.16e-07},
    "merge_dt9_c3_3x5_e0": {"vol": 0},
    "merge_dt9_c3_3x5_i0": {"vol": 0},
    "merge_dt9_c3_3x5_em": {"vol": 9.56e-08},
    "merge_dt9_c3_3x5_en": {"vol": 6.81e-09},
    "merge_dt9_c3_3x5_im": {"vol": 1.2e-07},
    "merge_dt9_c3_9x31_e0": {"vol": 0},
    "merge_dt9_c3_9x31_i0": {"vol": 0},
    "merge_dt9_c3_9x31_em": {"vol": 1.04e-07},
    "merge_dt9_c3_9x31_en": {"vol": 1.91e-09},
    "merge_dt9_c3_9x31_im": {"vol": 1.17e-07},
    "merge_dt9_c5_3x5_e0": {"vol": 0},
    "merge_dt9_c5_3x5_i0": {"vol": 0},
    "merge_dt9_c5_3x5_em": {"vol": 1.15e-07},
    "merge_dt9_c5_3x5_en": {"vol": 9.48e-09},
    "merge_dt9_c5_3x5_im": {"vol": 1.16e-07},
    "merge_dt9_c5_9x31_e0": {"vol": 0},
    "merge_dt9_c5_9x31_i0": {"vol": 0},
    "merge_dt9_c5_9x31_em": {"vol": 1.28e-07},
    "merge_dt9_c5_9x31_en": {"vol": 3.22e-09},
    "merge_dt9_c5_9x31_im": {"vol": 1.42e-07},
    "merge_dt14_c1_3x5_e0": {"vol": 0},
    "merge_dt14_c1_3x5_i0": {"vol": 0},
    "merge_dt14_c1_3x5_em": {"vol": 9.8e-08},
    "merge_dt14_c1_3x5_en": {"vol": 3.16e-09},
    "merge_dt14_c1_3x5_im": {"vol": 6.31e-08},
    "merge_dt14_c1_9x31_e0": {"vol": 0},
    "merge_dt14_c1_9x31_i0": {"vol": 0},
    "merge_dt14_c1_9x31_em": {"vol": 3.54e-08},
    "merge_dt14_c1_9x31_en": {"vol": 5.77e-11},
    "merge_dt14_c1_9x31_im": {"vol": 1.29e-07},
    "merge_dt14_c3_3x5_e0": {"vol": 0},
    "merge_dt14_c3_3x5_i0": {"vol": 0},
    "merge_dt14_c3_3x5_em": {"vol": 1.14e-07},
    "merge_dt14_c3_3x5_en": {"vol": 5.71e-09},
    "merge_dt14_c3_3x5_im": {"vol": 1.14e-07},
    "merge_dt14_c3_9x31_e0": {"vol": 0},
    "merge_dt14_c3_9x31_i0": {"vol": 0},
    "merge_dt14_c3_9x31_em": {"vol": 1.41e-07},
    "merge_dt14_c3_9x31_en": {"vol": 9.96e-09},
    "merge_dt14_c3_9x31_im": {"vol": 1.23e-07},
    "merge_dt14_c5_3x5_e0": {"vol": 0},
    "merge_dt14_c5_3x5_i0": {"vol": 0},
    "merge_dt14_c5_3x5_em": {"vol": 1.2e-07},
    "merge_dt14_c5_3x5_en": {"vol": 1.34e-08},
    "merge_dt14_c5_3x5_im": {"vol": 8.17e-08},
    "merge_dt14_c5_9x31_e0": {"vol": 0},
    "merge_dt14_c5_9x31_i0": {"vol": 0},
    "merge_dt14_c5_9x31_em": {"vol": 1.31e-07},
    "merge_dt14_c5_9x31_en": {"vol": 2.45e-09},
    "merge_dt14_c5_9x31_im": {"vol": 1.3e-07},
    "merge_dt15_c1_3x5_e0": {"vol": 0},
    "merge_dt15_c1_3x5_i0": {"vol": 0},
    "merge_dt15_c1_3x5_em": {"vol": 7.64e-08},
    "merge_dt15_c1_3x5_en": {"vol": 4.85e-09},
    "merge_dt15_c1_3x5_im": {"vol": 1.37e-07},
    "merge_dt15_c1_9x31_e0": {"vol": 0},
    "merge_dt15_c1_9x31_i0": {"vol": 0},
    "merge_dt15_c1_9x31_em": {"vol": 1.42e-07},
    "merge_dt15_c1_9x31_en": {"vol": 4e-10},
    "merge_dt15_c1_9x31_im": {"vol": 2e-07},
    "merge_dt15_c3_3x5_e0": {"vol": 0},
    "merge_dt15_c3_3x5_i0": {"vol": 0},
    "merge_dt15_c3_3x5_em": {"vol": 7.06e-08},
    "merge_dt15_c3_3x5_en": {"vol": 9.61e-10},
    "merge_dt15_c3_3x5_im": {"vol": 1.35e-07},
    "merge_dt15_c3_9x31_e0": {"vol": 0},
    "merge_dt15_c3_9x31_i0": {"vol": 0},
    "merge_dt15_c3_9x31_em": {"vol": 1.39e-07},
    "merge_dt15_c3_9x31_en": {"vol": 9.05e-09},
    "merge_dt15_c3_9x31_im": {"vol": 8.71e-08},
    "merge_dt15_c5_3x5_e0": {"vol": 0},
    "merge_dt15_c5_3x5_i0": {"vol": 0},
    "merge_dt15_c5_3x5_em": {"vol": 1.02e-07},
    "merge_dt15_c5_3x5_en": {"vol": 4.43e-09},
    "merge_dt15_c5_3x5_im": {"vol": 7.7e-08},
    "merge_dt15_c5_9x31_e0": {"vol": 0},
    "merge_dt15_c5_9x31_i0": {"vol": 0},
    "merge_dt15_c5_9x31_em": {"vol": 1.23e-07},
    "merge_dt15_c5_9x31_en": {"vol": 3.69e-09},
    "merge_dt15_c5_9x31_im": {"vol": 1.42e-07},
    "merge_dt20_c1_3x5_e0": {"vol": 0},
    "merge_dt20_c1_3x5_i0": {"vol": 0},
    "merge_dt20_c1_3x5_em": {"vol": 1.14e-07},
    "merge_dt20_c1_3x5_en": {"vol": 3.01e-11},
    "merge_dt20_c1_3x5_im": {"vol": 4.71e-08},
    "merge_dt20_c1_9x31_e0": {"vol": 0},
    "merge_dt20_c1_9x31_i0": {"vol": 0},
    "merge_dt20_c1_9x31_em": {"vol": 1.12e-07},
    "merge_dt20_c1_9x31_en": {"vol": 8.54e-10},
    "merge_dt20_c1_9x31_im": {"vol": 1.1e-08},
    "merge_dt20_c3_3x5_e0": {"vol": 0},
    "merge_dt20_c3_3x5_i0": {"vol": 0},
    "merge_dt20_c3_3x5_em": {"vol": 1.22e-07},
    "merge_dt20_c3_3x5_en": {"vol": 2.79e-09},
    "merge_dt20_c3_3x5_im": {"vol": 1.18e-07},
    "merge_dt20_c3_9x31_e0": {"vol": 0},
    "merge_dt20_c3_9x31_i0": {"vol": 0},
    "merge_dt20_c3_9x31_em": {"vol": 1.36e-07},
    "merge_dt20_c3_9x31_en": {"vol": 6.51e-10},
    "merge_dt20_c3_9x31_im": {"vol": 1.44e-07},
    "merge_dt20_c5_3x5_e0": {"vol": 0},
    "merge_dt20_c5_3x5_i0": {"vol": 0},
    "merge_dt20_c5_3x5_em": {"vol": 1.86e-07},
    "merge_dt20_c5_3x5_en": {"vol": 5.43e-09},
    "merge_dt20_c5_3x5_im": {"vol": 1.18e-07},
    "merge_dt20_c5_9x31_e0": {"vol": 0},
    "merge_dt20_c5_9x31_i0": {"vol": 0},
    "merge_dt20_c5_9x31_em": {"vol": 1.34e-07},
    "merge_dt20_c5_9x31_en": {"vol": 1.72e-09},
    "merge_dt20_c5_9x31_im": {"vol": 1.4e-07},
    "resize_3x5x7_to_3x5x7_a0_add": {"out": 5.69e-08},
    "resize_3x5x7_to_3x5x7_a0_noadd": {"out": 0},
    "resize_3x5x7_to_3x5x7_a1_add": {"out": 9.39e-08},
    "resize_3x5x7_to_3x5x7_a1_noadd": {"out": 5.67e-08},
    "resize_2x5x7_to_4x9x13_a0_add": {"out": 6.69e-08},
    "resize_2x5x7_to_4x9x13_a0_noadd": {"out": 7.55e-08},
    "resize_2x5x7_to_4x9x13_a1_add": {"out": 1.37e-07},
    "resize_2x5x7_to_4x9x13_a1_noadd": {"out": 1.22e-07},
    "resize_3x9x15_to_5x17x30_a0_add": {"out": 6.86e-07},
    "resize_3x9x15_to_5x17x30_a0_noadd": {"out": 1.03e-06},
    "resize_3x9x15_to_5x17x30_a1_add": {"out": 5.47e-07},
    "resize_3x9x15_to_5x17x30_a1_noadd": {"out": 9.59e-07},
    "resize_1x1x1_to_3x4x5_a0_add": {"out": 4.98e-08},
    "resize_1x1x1_to_3x4x5_a0_noadd": {"out": 0},
    "resize_1x1x1_to_3x4x5_a1_add": {"out": 1.1e-07},
    "resize_1x1x1_to_3x4x5_a1_noadd": {"out": 1.05e-07},
    "resize_3x4x5_to_1x1x1_a0_add": {"out": 2.39e-08},
    "resize_3x4x5_to_1x1x1_a0_noadd": {"out": 0},
    "resize_3x4x5_to_1x1x1_a1_add": {"out": 8e-08},
    "resize_3x4x5_to_1x1x1_a1_noadd": {"out": 1.2e-07},
    "resize_4x6x8_to_1x6x1_a0_add": {"out": 3.72e-08},
    "resize_4x6x8_to_1x6x1_a0_noadd": {"out": 0},
    "resize_4x6x8_to_1x6x1_a1_add": {"out": 9.32e-08},
    "resize_4x6x8_to_1x6x1_a1_noadd": {"out": 8.3e-08},
    "resize_5x9x13_to_3x5x7_a0_add": {"out": 3.91e-08},
    "resize_5x9x13_to_3x5x7_a0_noadd": {"out": 0},
    "resize_5x9x13_to_3x5x7_a1_add": {"out": 1.03e-07},
    "resize_5x9x13_to_3x5x7_a1_noadd": {"out": 9.3e-08},
    "resize_3x100x150_to_6x200x300_a1_add": {"out": 6.68e-06},
    "resizebwd_3x5x7_to_3x5x7_a0_add+g": {"grad_a": 0, "grad_add": 0},
    "resizebwd_3x5x7_to_3x5x7_a0_add": {"grad_a": 0, "grad_add": 0},
    "resizebwd_3x5x7_to_3x5x7_a0_none": {"grad_a": 0, "grad_add": 0},
    "resizebwd_3x5x7_to_3x5x7_a1_add+g": {"grad_a": 8.24e-08, "grad_add": 8.24e-08},
    "resizebwd_3x5x7_to_3x5x7_a1_add": {"grad_a": 8.24e-08, "grad_add": 8.24e-08},
    "resizebwd_3x5x7_to_3x5x7_a1_none": {"grad_a": 9.99e-08, "grad_add": 9.99e-08},
    "resizebwd_2x5x7_to_4x9x13_a0_add+g": {"grad_a": 7.64e-08, "grad_add": 0},
    "resizebwd_2x5x7_to_4x9x13_a0_add": {"grad_a": 7.64e-08, "grad_add": 0},
    "resizebwd_2x5x7_to_4x9x13_a0_none": {"grad_a": 7.64e-08, "grad_add": 0},
    "resizebwd_2x5x7_to_4x9x13_a1_add+g": {"grad_a": 1.25e-07, "grad_add": 7.69e-08},
    "resizebwd_2x5x7_to_4x9x13_a1_add": {"grad_a": 1.25e-07, "grad_add": 7.69e-08},
    "resizebwd_2x5x7_to_4x9x13_a1_none": {"grad_a": 8.13e-08, "grad_add": 9.54e-08},
    "resizebwd_3x9x15_to_5x17x30_a0_add+g": {"grad_a": 7e-07, "grad_add": 0},
    "resizebwd_3x9x15_to_5x17x30_a0_add": {"grad_a": 7e-07, "grad_add": 0},
    "resizebwd_3x9x15_to_5x17x30_a0_none": {"grad_a": 7e-07, "grad_add": 0},
    "resizebwd_3x9x15_to_5x17x30_a1_add+g": {"grad_a": 6.08e-07, "grad_add": 7.9e-07},
    "resizebwd_3x9x15_to_5x17x30_a1_add": {"grad_a": 6.08e-07, "grad_add": 7.9e-07},
    "resizebwd_3x9x15_to_5x17x30_a1_none": {"grad_a": 7.2e-07, "grad_add": 7.33e-07},
    "resizebwd_1x1x1_to_3x4x5_a0_add+g": {"grad_a": 6.98e-08, "grad_add": 0},
    "resizebwd_1x1x1_to_3x4x5_a0_add": {"grad_a": 6.98e-08, "grad_add": 0},
    "resizebwd_1x1x1_to_3x4x5_a0_none": {"grad_a": 6.98e-08, "grad_add": 0},
    "resizebwd_1x1x1_to_3x4x5_a1_add+g": {"grad_a": 1.18e-07, "grad_add": 7.16e-08},
    "resizebwd_1x1x1_to_3x4x5_a1_add": {"grad_a": 1.18e-07, "grad_add": 7.16e-08},
    "resizebwd_1x1x1_to_3x4x5_a1_none": {"grad_a": 5.8e-08, "grad_add": 4.64e-08},
    "resizebwd_3x4x5_to_1x1x1_a0_add+g": {"grad_a": 0, "grad_add": 0},
    "resizebwd_3x4x5_to_1x1x1_a0_add": {"grad_a": 0, "grad_add": 0},
    "resizebwd_3x4x5_to_1x1x1_a0_none": {"grad_a": 0, "grad_add": 0},
    "resizebwd_3x4x5_to_1x1x1_a1_add+g": {"grad_a": 3.8e-08, "grad_add": 3.8e-08},
    "resizebwd_3x4x5_to_1x1x1_a1_add": {"grad_a": 3.8e-08, "grad_add": 3.8e-08},
    "resizebwd_3x4x5_to_1x1x1_a1_none": {"grad_a": 5.64e-08, "grad_add": 5.64e-08},
    "resizebwd_4x6x8_to_1x6x1_a0_add+g": {"grad_a": 0, "grad_add": 0},
    "resizebwd_4x6x8_to_1x6x1_a0_add": {"grad_a": 0, "grad_add": 0},
    "resizebwd_4x6x8_to_1x6x1_a0_none": {"grad_a": 0, "grad_add": 0},
    "resizebwd_4x6x8_to_1x6x1_a1_add+g": {"grad_a": 5.36e-08, "grad_add": 5.36e-08},
    "resizebwd_4x6x8_to_1x6x1_a1_add": {"grad_a": 5.36e-08, "grad_add": 5.36e-08},
    "resizebwd_4x6x8_to_1x6x1_a1_none": {"grad_a": 7.36e-08, "grad_add": 7.36e-08},
    "resizebwd_5x9x13_to_3x5x7_a0_add+g": {"grad_a": 0, "grad_add": 0},
    "resizebwd_5x9x13_to_3x5x7_a0_add": {"grad_a": 0, "grad_add": 0},
    "resizebwd_5x9x13_to_3x5x7_a0_none": {"grad_a": 0, "grad_add": 0},
    "resizebwd_5x9x13_to_3x5x7_a1_add+g": {"grad_a": 4.69e-08, "grad_add": 4.69e-08},
    "resizebwd_5x9x13_to_3x5x7_a1_add": {"grad_a": 4.69e-08, "grad_add": 4.69e-08},
    "resizebwd_5x9x13_to_3x5x7_a1_none": {"grad_a": 5.46e-08, "grad_add": 5.46e-08},
    "bilinear_17x30_to_8x15_s1": {"out": 1.81e-06},
    "bilinear_17x30_to_8x15_s2.5": {"out": 1.8e-06},
    "bilinear_5x7_to_5x7_s1": {"out": 0},
    "bilinear_5x7_to_5x7_s2.5": {"out": 3.97e-08},
    "bilinear_1x5_to_4x9_s1": {"out": 3.92e-08},
    "bilinear_1x5_to_4x9_s2.5": {"out": 2.35e-08},
    "bilinear_5x1_to_4x3_s1": {"out": 1.26e-07},
    "bilinear_5x1_to_4x3_s2.5": {"out": 1.06e-07},
    "bilinear_4x6_to_1x1_s1": {"out": 0},
    "bilinear_4x6_to_1x1_s2.5": {"out": 4.37e-08},
    "bilinear_6x9_to_13x20_s1": {"out": 4.03e-07},
    "bilinear_6x9_to_13x20_s2.5": {"out": 4.2e-07},
    "bilinear_pair_17x30_to_8x15": {"map0": 1.81e-06, "map1": 1.61e-06},
    "bilinear_pair_5x7_to_5x7": {"map0": 0, "map1": 4.39e-08},
    "bilinear_pair_1x5_to_4x9": {"map0": 3.92e-08, "map1": 1.99e-08},
    "bilinear_pair_5x1_to_4x3": {"map0": 1.26e-07, "map1": 1.63e-07},
    "bilinear_pair_4x6_to_1x1": {"map0": 0, "map1": 3.84e-08},
    "bilinear_pair_6x9_to_13x20": {"map0": 4.03e-07, "map1": 4.4e-07},
    "range_5x7_r4": {"low": 2.73e-09, "high": 3.69e-08, "cand": 3.69e-08},
    "range_5x7_r0": {"low": 0, "high": 0, "cand": 0},
    "range_5x7_r-2": {"low": 3.84e-08, "high": 0, "cand": 3.84e-08},
    "range_9x31_r4": {"low": 2.71e-09, "high": 3.67e-08, "cand": 3.67e-08},
    "range_9x31_r0": {"low": 0, "high": 0, "cand": 0},
    "range_9x31_r-2": {"low": 3.82e-08, "high": 1.3e-09, "cand": 3.82e-08},
    "unet_5x7x15x24_x1": {"out": 0.0261, "grad_logits": 0.0113, "grad_disp": 0.0219},
    "unet_5x7x15x24_x30": {"out": 0.0231, "grad_logits": 0.0094, "grad_disp": 0.0163},
    "unet_6x9x12x20_x1": {"out": 0.0192, "grad_logits": 0.00746, "grad_disp": 0.0057},
    "unet_6x9x12x20_x30": {"out": 0.0293, "grad_logits": 0.00587, "grad_disp": 0.00797},
    "unet_4x8x4x8_x1": {"out": 0.00964, "grad_logits": 0.00293, "grad_disp": 0.00113},
    "unet_4x8x4x8_x30": {"out": 0.00388, "grad_logits": 0.00185, "grad_disp": 0.000758},
    "unet_4x8x12x24_x1": {"out": 0.0811, "grad_logits": 0.0235, "grad_disp": 0.0219},
    "unet_4x8x12x24_x30": {"out": 0.221, "grad_logits": 0.00998, "grad_disp": 0.0434},
    "unet_1x5x4x20_x1": {"out": 0.00966, "grad_logits": 0.00254, "grad_disp": 0.00306},
    "unet_1x5x4x20_x30": {"out": 0.00996, "grad_logits": 0.00442, "grad_disp": 0.00281},
    "unet_5x1x20x4_x1": {"out": 0.0111, "grad_logits": 0.003, "grad_disp": 0.00446},
    "unet_5x1x20x4_x30": {"out": 0.00902, "grad_logits": 0.00845, "grad_disp": 0.0029},
    "unet_3x5x7x10_x1": {"out": 0.0102, "grad_logits": 0.00371, "grad_disp": 0.00252},
    "unet_3x5x7x10_x30": {"out": 0.00771, "grad_logits": 0.00405, "grad_disp": 0.00338},
    "convex_1x6x2_x1": {"out": 0.0122, "grad_logits": 0.00335, "grad_disp": 0.01},
    "convex_1x6x2_x30": {"out": 0.00884, "grad_logits": 0.144, "grad_disp": 0.000683},
    "convex_5x1x2_x1": {"out": 0.0148, "grad_logits": 0.00248, "grad_disp": 0.00147},
    "convex_5x1x2_x30": {"out": 0.00824, "grad_logits": 0.282, "grad_disp": 0.000493},
    "convex_4x5x1_x1": {"out": 0.0164, "grad_logits": 0.138, "grad_disp": 0.00268},
    "convex_4x5x1_x30": {"out": 0.00865, "grad_logits": 0.131, "grad_disp": 0.000545},
    "convex_3x4x3_x1": {"out": 0.028, "grad_logits": 0.164, "grad_disp": 0.00957},
    "convex_3x4x3_x30": {"out": 0.00903, "grad_logits": 0.429, "grad_disp": 0.00467},
}


if __name__ == "__main__":
    for key, (fn, case) in measured().items():
        print('    "%s": {%s},' % (key, ", ".join('"%s": %.3g' % kv for kv in fn(case).items())))
