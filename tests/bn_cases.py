"""Test infrastructure: the cases of tests/test_batchnorm_gpu.py -- shapes, layouts, channel contents -- with the error metric, the
fp32 yardstick and the bounds, shared with tests/test_batchnorm_ref_cpu.py (which pins the yardstick figures written below and shows
that the bounds notice planted errors).  No GPU in here.

Metric.  Every error is taken PER CHANNEL, relative to the size of the reference in that channel (never larger than the tensor's
maximum, so no weaker than "relative to the tensor's max" of test_fused_conv_batchnorm_activation_matches_framework):
  out, dx            max |got - ref| over the channel's planes / max |ref| over the channel's planes
  s1, s2             |got - ref| / max_c |ref|            (sums of normalised terms: one scale for all channels)
  mean               |got - ref| / max(|mean|, std)       var: / var
  running_mean'      / max(|running_mean|, |mean|, std)   running_var': / max(running_var, unbiased var)
A reference that is exactly 0 (the output of a constant channel with beta == 0, its var, its s2) has to be met exactly.

Bounds.  BASE holds for every well-conditioned channel (|mean| <= 5 std, gamma in [0.5, 1.5], a typical first element): 5e-6 for
outputs, 2e-5 for gradients (dx, s1, s2), 1e-5 for statistics (mean, var, running).  For the other channels -- |mean| >> std, tiny
std, constant, outlier first element, gamma = 40 -- the bound of out / dx / s1,s2 is max(BASE, 4 x yardstick), the yardstick being
the error of the plain fp32 two-pass form on the same input (`yardstick_terms`: fp64 statistics rounded to fp32, then x * sc + sh and the
dx formula in fp32): what ANY fp32 implementation that stores mean / var as fp32 carries; the factor 4 leaves room for summation
order and the ~1.5 ulp sigmoid_fast.  Statistics stay at BASE everywhere: rounding mean / var to fp32 is 6e-8 of themselves.
YARD holds the measured yardstick per case and kind of hard channel; `python tests/bn_cases.py` prints it.
"""
import collections

import numpy as np
import torch

import bn_ref
import synth

TINY = 1e-30
BASE = {"out": 5e-6, "grad": 2e-5, "stat": 1e-5}
GUARD = 64                      # sentinel elements in front of the first and behind the last plane (a multiple of 4)
SENTINEL = -777.25

# channel contents: mean + std * N(0,1);  "const" / "cneg": every element 4.0 / -0.5 (powers of two, so that mean * sc is exact in fp32
# and, with beta == 0, z is exactly 0 whichever way the compiler contracts x * sc + sh: a constant channel amplifies the rounding of
# sh by 1 / sqrt(eps), so any other value tests the compiler's choice);  "pivot": (3,1) with the first element at mean + 30 std
KINDS = {"n01": (0.0, 1.0), "n31": (3.0, 1.0), "m50": (-50.0, 1.0), "k1000": (1000.0, 1.0), "tiny": (0.0, 0.01), "wide": (5.0, 30.0),
         "const": (4.0, 0.0), "cneg": (-0.5, 0.0), "pivot": (3.0, 1.0)}
ALL_KINDS = ("n01", "k1000", "pivot", "m50", "tiny", "const", "n31", "wide")
WELL = ("n01", "n31", "wide")

Case = collections.namedtuple("Case", "name form shape layout act kinds gamma affine momentum running")
# form: "small" = the default one-launch bound, "two" = ts_bn_set_small_elems(0) (and the three-launch form beside it)
# gamma: "unit" = uniform [0.5, 1.5], beta N(0, 0.2) (0 on a constant channel);  "g40" = 40 everywhere, beta 0
# affine False: null gamma / beta;  running False: null running pointers and a null counter


def _cases():
    out = []
    acts = (bn_ref.ACT_NONE, bn_ref.ACT_SILU, bn_ref.ACT_RELU)
    for form, shape, kinds in (("small", (2, 3, 1024), ("n01", "k1000", "pivot")), ("two", (2, 3, 2136), ("m50", "tiny", "const"))):
        for layout in range(4):
            for act in acts:
                out.append(Case("%s_%dx%dx%d_L%d_a%d" % ((form,) + shape + (layout, act)), form, shape, layout, act, kinds, "unit", True,
                                (0.1, 0.0, 1.0)[(layout + act) % 3], True))
    for form, shape, layout, act, kinds, gamma, affine, momentum, running in (
            ("small", (2, 3, 1023), 2, 2, ("wide", "const", "m50"), "unit", True, 0.1, True),
            ("small", (3, 5, 77), 3, 1, ("pivot", "tiny", "n31", "k1000", "n01"), "unit", True, 1.0, True),
            ("small", (1, 2, 1), 0, 0, ("const", "cneg"), "unit", True, 0.1, True),           # B * N == 1: every channel is constant
            ("small", (1, 4, 10240), 0, 1, ("n01", "pivot", "tiny", "wide"), "unit", True, 1.0, True),      # exactly kSmallElems
            ("small", (1, 4, 10244), 1, 2, ("n31", "k1000", "const", "pivot"), "unit", True, 1.0, True),    # just over: two launches
            ("two", (2, 3, 2135), 3, 1, ("pivot", "n01", "k1000"), "unit", True, 0.1, True),
            ("two", (1, 1, 4100), 2, 0, ("pivot",), "unit", True, 0.1, True),                 # five chunks, a short last one
            ("two", (1, 2, 1028), 0, 2, ("pivot", "tiny"), "unit", True, 0.0, True),               # the outlier on the float4 two-launch path
            ("two", (4, 300, 8), 3, 1, ALL_KINDS, "unit", True, 0.1, True),                   # B * C > 1024: one chunk, short planes
            ("small", (2, 3, 1024), 0, 1, ("n01", "const", "n31"), "g40", True, 0.1, True),   # z over +-160: both SiLU saturation branches
            ("two", (2, 3, 2136), 0, 2, ("n31", "const", "tiny"), "g40", True, 0.1, True),
            ("small", (2, 3, 1023), 1, 1, ("n01", "pivot", "tiny"), "unit", False, 0.1, True),        # null gamma / beta
            ("two", (1, 2, 1028), 3, 1, ("n31", "const"), "unit", False, 0.1, False),                 # ... and null running / counter
            ("small", (3, 5, 77), 0, 2, ("n01", "wide", "m50", "n31", "const"), "unit", True, 0.1, False)):
        tag = "%s_%dx%dx%d_L%d_a%d%s%s%s" % ((form,) + shape + (layout, act, "_g40" if gamma == "g40" else "", "" if affine else "_noaffine",
                                                                 "" if running else "_norunning"))
        out.append(Case(tag, form, shape, layout, act, kinds, gamma, affine, momentum, running))
    assert len({c.name for c in out}) == len(out)
    return out


CASES = _cases()


def case_kinds(case):
    C = case.shape[1]
    return [case.kinds[c % len(case.kinds)] for c in range(C)]


def case_eps(case):
    """1e-5 (the framework's default) where a tiny-std or constant channel makes it matter; 1e-3 elsewhere, so that an eps on the
    wrong side of the square root moves a unit-variance channel by 5e-4 and not by 5e-6 (the sensitivity checks need that)"""
    return 1e-5 if {"tiny", "const"} & set(case_kinds(case)) else 1e-3


def hard_channels(case):
    """[C] bool: the channels whose bound comes from the yardstick"""
    return torch.tensor([case.gamma == "g40" or k not in WELL for k in case_kinds(case)])


def channel_data(seed, tag, kinds, B, N):
    """x [B, C, N] fp32 with the listed channel contents"""
    C = len(kinds)
    x = np.empty((B, C, N), np.float32)
    for c, k in enumerate(kinds):
        mean, std = KINDS[k]
        x[:, c] = np.float32(mean) + np.float32(std) * synth.normal(seed, "%s%d" % (tag, c), (B, N))
        if k == "pivot":
            x[0, c, 0] = mean + 30.0 * std
    return torch.from_numpy(x)


def make_inputs(case):
    B, C, N = case.shape
    seed = 900 + CASES.index(case)
    kinds = case_kinds(case)
    d = {"x": channel_data(seed, "x", kinds, B, N), "dy": torch.from_numpy(synth.normal(seed, "dy", (B, C, N))),
         "eps": case_eps(case), "momentum": case.momentum, "gamma": None, "beta": None, "running": None}
    if case.affine:
        if case.gamma == "g40":
            d["gamma"], d["beta"] = torch.full((C,), 40.0), torch.zeros(C)
        else:
            d["gamma"] = torch.from_numpy(synth.uniform(seed, "g", (C,), 0.5, 1.5))
            d["beta"] = torch.from_numpy(synth.normal(seed, "b", (C,), 0.2))
            d["beta"][torch.tensor([KINDS[k][1] == 0.0 for k in kinds])] = 0.0
    if case.running:
        d["running"] = (torch.from_numpy(synth.normal(seed, "rm", (C,), 0.2)), torch.from_numpy(synth.uniform(seed, "rv", (C,), 0.5, 1.5)))
    return d


def layout_of(case, which):
    """(offset, bstride, cstride) in elements of tensor `which` (x | out | dy | dx) behind the GUARD; dx shares x's strides (C ABI)"""
    B, C, N = case.shape
    L = case.layout
    if L == 0:                                  # contiguous, 16-byte aligned
        return 0, C * N, N
    if L == 1:                                  # misaligned bases (x by one element): the scalar kernels, whatever N is
        return {"x": 1, "out": 2, "dy": 0, "dx": 3}[which], C * N, N
    if L == 2:                                  # a channel stride that is no multiple of 4
        return 0, C * (N + 2), N + 2
    if which in ("x", "dx"):                    # padded, multiples of 4: the float4 kernels where N % 4 == 0
        return 0, C * (N + 8) + 16, N + 8
    return 0, C * (N + 12) + 4, N + 12          # ... and other strides for out / dy than for x


# ---- eval mode and the cross-rank merge -------------------------------------------------------------------------------------------
EVAL_CASES = [Case("eval_%dx%dx%d_L%d_a%d" % (s + (L, a)), "eval", s, L, a, kinds, "unit", aff, 0.0, False)
              for s, L, a, kinds, aff in (((2, 3, 1024), 3, 1, ("n01", "n31", "wide"), True), ((2, 3, 1023), 1, 2, ("wide", "n01", "n31"), True),
                                          ((3, 5, 77), 2, 0, ("n31", "wide", "n01"), False), ((1, 2, 2136), 0, 1, ("n01", "n31"), True))]


def eval_inputs(case):
    """a well-conditioned case with `mean` / `var` that are NOT the batch's: running statistics somewhere near them"""
    B, C, N = case.shape
    seed = 700 + EVAL_CASES.index(case)
    kinds = case_kinds(case)
    d = {"x": channel_data(seed, "x", kinds, B, N), "dy": torch.from_numpy(synth.normal(seed, "dy", (B, C, N))), "eps": 1e-3, "gamma": None, "beta": None}
    m0 = torch.tensor([KINDS[k][0] for k in kinds])
    s0 = torch.tensor([KINDS[k][1] for k in kinds])
    d["mean"] = m0 + s0 * torch.from_numpy(synth.normal(seed, "m", (C,), 0.5))
    d["var"] = s0 * s0 * torch.from_numpy(synth.uniform(seed, "v", (C,), 0.5, 2.0))
    if case.affine:
        d["gamma"] = torch.from_numpy(synth.uniform(seed, "g", (C,), 0.5, 1.5))
        d["beta"] = torch.from_numpy(synth.normal(seed, "b", (C,), 0.2))
    return d


MERGE_COUNTS = {1: (405.0,), 2: (405.0, 8160.0), 3: (405.0, 8160.0, 1.0), 5: (405.0, 8160.0, 1.0, 77.0, 2048.0)}


def merge_records(world, C):
    """per rank (mean [C], var [C], count): rank means several std apart, unequal counts"""
    recs = []
    for r in range(world):
        mean = torch.from_numpy(synth.normal(300 + r, "mm%d" % C, (C,), 1.0)) + 4.0 * r
        var = torch.from_numpy(synth.uniform(300 + r, "mv%d" % C, (C,), 0.5, 2.0))
        recs.append((mean, var if MERGE_COUNTS[world][r] > 1 else torch.zeros(C), MERGE_COUNTS[world][r]))
    return recs


# ---- metric ----------------------------------------------------------------------------------------------------------------------
def chan_max(t):
    return t.abs().amax(dim=(0, 2))


def err_planes(got, ref):
    """[C]: out / dx"""
    return chan_max(got.double().cpu() - ref) / chan_max(ref).clamp_min(TINY)


def err_vec(got, ref, scale):
    return (got.double().cpu() - ref).abs() / scale.clamp_min(TINY)


def stat_scales(mean, var, count, running):
    """the four scales of mean, var, running_mean', running_var' (running: the values BEFORE the update, or None)"""
    std = var.sqrt()
    unb = var * (count / (count - 1.0)) if count > 1 else var
    sm = torch.maximum(mean.abs(), std)
    if running is None:
        return sm, var, None, None
    return sm, var, torch.maximum(running[0].double().abs(), sm), torch.maximum(running[1].double(), unb)


# ---- the fp32 yardstick ----------------------------------------------------------------------------------------------------------
def _sigmoid32(z):
    return torch.sigmoid(z.double()).float()            # correctly rounded: the same figure on every host


def yardstick_terms(x, dy, mean, var, gamma, beta, eps, act, train, count):
    """The plain fp32 two-pass form: mean / var (fp64) rounded to fp32, everything after it in fp32 torch (sums in fp64, rounded).
    -> out, dx, s1, s2 (fp32)"""
    B, C, N = x.shape
    f = lambda v, fill: (torch.full((C,), fill) if v is None else v.float()).view(1, C, 1)
    m, g, b = mean.float().view(1, C, 1), f(gamma, 1.0), f(beta, 0.0)
    inv = (1.0 / (var.float() + torch.tensor(eps, dtype=torch.float32)).double().sqrt()).float().view(1, C, 1)
    sc = inv * g
    sh = b - m * sc
    z = x * sc + sh
    out = z * _sigmoid32(z) if act == bn_ref.ACT_SILU else z.clamp_min(0.0) if act == bn_ref.ACT_RELU else z
    xh = (x - m) * inv
    zz = xh * g + b
    if act == bn_ref.ACT_SILU:
        s = _sigmoid32(zz)
        gr = s * (1.0 + zz * (1.0 - s))
    elif act == bn_ref.ACT_RELU:
        gr = (zz > 0).float()
    else:
        gr = torch.ones_like(zz)
    dz = dy * gr
    s1, s2 = dz.double().sum(dim=(0, 2)).float(), (dz * xh).double().sum(dim=(0, 2)).float()
    if train:
        inv_n = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(count, dtype=torch.float32)
        dx = (dz - (s1 * inv_n).view(1, C, 1) - xh * (s2 * inv_n).view(1, C, 1)) * inv * g
    else:
        dx = dz * inv * g
    return out, dx, s1, s2


def reference(case, d=None):
    """the float64 results of a case: dict out, mean, var, running, dx, s1, s2"""
    d = d or make_inputs(case)
    B, C, N = case.shape
    out, mean, var, running = bn_ref.bn_act_fwd(d["x"], d["gamma"], d["beta"], d["eps"], case.act, momentum=d["momentum"], running=d["running"])
    dx, s1, s2 = bn_ref.bn_act_bwd(d["x"], d["dy"], mean, var, d["gamma"], d["beta"], d["eps"], case.act, True, B * N)
    return {"out": out, "mean": mean, "var": var, "running": running, "dx": dx, "s1": s1, "s2": s2}


def errors(got, ref):
    """per-channel errors of out, dx, s1, s2 in the metric of this file -> dict of [C]"""
    return {"out": err_planes(got["out"], ref["out"]), "dx": err_planes(got["dx"], ref["dx"]),
            "s1": err_vec(got["s1"], ref["s1"], ref["s1"].abs().max()), "s2": err_vec(got["s2"], ref["s2"], ref["s2"].abs().max())}


def measure(case):
    """{kind: (out, dx, s)}: the yardstick's error on the case's input for each hard kind of channel in it (maximum over that kind's
    channels; s = the larger of s1's and s2's)"""
    hard = hard_channels(case)
    if not bool(hard.any()):
        return {}
    d = make_inputs(case)
    ref = reference(case, d)
    B, C, N = case.shape
    o, dx, s1, s2 = yardstick_terms(d["x"], d["dy"], ref["mean"], ref["var"], d["gamma"], d["beta"], d["eps"], case.act, True, B * N)
    e = errors({"out": o, "dx": dx, "s1": s1, "s2": s2}, ref)
    kinds, res = case_kinds(case), {}
    for k in dict.fromkeys(kinds):
        sel = hard & torch.tensor([kk == k for kk in kinds])
        if bool(sel.any()):
            res[k] = (float(e["out"][sel].max()), float(e["dx"][sel].max()), float(torch.maximum(e["s1"], e["s2"])[sel].max()))
    return res


# measured yardstick per case and hard kind of channel: (out, dx, s1 / s2).  The bound of such a channel is max(BASE, 4 x this): where
# 4 x the figure is below BASE (5e-6 | 2e-5 | 2e-5) the bound IS the base bound.  Behind each line: the bounds that differ from BASE.
YARD = {
    "small_2x3x1024_L0_a0": {"k1000": (1.58e-05, 4.07e-07, 1.18e-05), "pivot": (8.24e-08, 7.48e-08, 6.42e-08)},    # k1000 out 6.33e-05, k1000 s 4.71e-05
    "small_2x3x1024_L0_a1": {"k1000": (2.04e-05, 1.15e-05, 1.13e-05), "pivot": (1.97e-08, 1.12e-07, 3e-08)},    # k1000 out 8.15e-05, k1000 dx 4.58e-05, k1000 s 4.5e-05
    "small_2x3x1024_L0_a2": {"k1000": (2.81e-05, 1.76e-07, 3.66e-06), "pivot": (5.28e-08, 8.72e-08, 2.09e-09)},    # k1000 out 0.000112
    "small_2x3x1024_L1_a0": {"k1000": (2.95e-05, 7.06e-07, 1.92e-05), "pivot": (1.59e-08, 1.02e-07, 4.84e-08)},    # k1000 out 0.000118, k1000 s 7.66e-05
    "small_2x3x1024_L1_a1": {"k1000": (2.04e-05, 9.9e-06, 2.06e-05), "pivot": (1.19e-08, 1.12e-07, 9.86e-08)},    # k1000 out 8.18e-05, k1000 dx 3.96e-05, k1000 s 8.24e-05
    "small_2x3x1024_L1_a2": {"k1000": (1.3e-05, 1.42e-07, 2.58e-06), "pivot": (1.87e-08, 1.06e-07, 1.59e-08)},    # k1000 out 5.22e-05
    "small_2x3x1024_L2_a0": {"k1000": (1.72e-05, 1.35e-07, 4.08e-06), "pivot": (7.94e-08, 1.41e-07, 7.16e-08)},    # k1000 out 6.89e-05
    "small_2x3x1024_L2_a1": {"k1000": (1.83e-05, 9.09e-06, 1.29e-05), "pivot": (1.52e-08, 1.19e-07, 3.47e-08)},    # k1000 out 7.33e-05, k1000 dx 3.63e-05, k1000 s 5.17e-05
    "small_2x3x1024_L2_a2": {"k1000": (2.13e-05, 3.89e-07, 1.07e-05), "pivot": (4.46e-08, 8.29e-08, 2.42e-08)},    # k1000 out 8.5e-05, k1000 s 4.27e-05
    "small_2x3x1024_L3_a0": {"k1000": (2.12e-05, 1.64e-07, 2.49e-06), "pivot": (6.2e-08, 9.94e-08, 3.24e-08)},    # k1000 out 8.47e-05
    "small_2x3x1024_L3_a1": {"k1000": (2.55e-05, 1.17e-05, 3e-06), "pivot": (7.55e-08, 1.87e-07, 2.33e-08)},    # k1000 out 0.000102, k1000 dx 4.66e-05
    "small_2x3x1024_L3_a2": {"k1000": (3.48e-05, 3.15e-07, 6.62e-06), "pivot": (8.37e-09, 8.15e-08, 4.6e-08)},    # k1000 out 0.000139, k1000 s 2.65e-05
    "two_2x3x2136_L0_a0": {"m50": (1.63e-06, 6.72e-08, 2.36e-07), "tiny": (7.94e-08, 1.38e-07, 2.93e-08), "const": (0, 1.06e-07, 5.63e-10)},    # m50 out 6.51e-06
    "two_2x3x2136_L0_a1": {"m50": (1.57e-06, 8.81e-07, 2.12e-06), "tiny": (1.07e-07, 1.71e-07, 2.78e-07), "const": (0, 1.07e-07, 5.36e-10)},    # m50 out 6.29e-06
    "two_2x3x2136_L0_a2": {"m50": (6.81e-07, 7.97e-08, 2.46e-07), "tiny": (6.68e-08, 1.1e-07, 5.62e-08), "const": (0, 0, 0)},
    "two_2x3x2136_L1_a0": {"m50": (8.97e-07, 1.27e-07, 3.64e-08), "tiny": (5.52e-08, 8.3e-08, 1.15e-07), "const": (0, 1.19e-07, 3.65e-08)},
    "two_2x3x2136_L1_a1": {"m50": (6.13e-07, 1.62e-07, 6.02e-08), "tiny": (1.61e-07, 1.38e-07, 5.86e-08), "const": (0, 1.18e-07, 8.8e-10)},
    "two_2x3x2136_L1_a2": {"m50": (6.43e-07, 1.06e-07, 2.09e-07), "tiny": (7.5e-08, 1.13e-07, 8.26e-08), "const": (0, 0, 0)},
    "two_2x3x2136_L2_a0": {"m50": (1.5e-06, 1.07e-07, 3.47e-07), "tiny": (7.07e-08, 1.08e-07, 6.45e-08), "const": (0, 9.06e-08, 3.07e-08)},    # m50 out 6e-06
    "two_2x3x2136_L2_a1": {"m50": (6.92e-07, 5.79e-07, 1.21e-06), "tiny": (9.63e-08, 1.27e-07, 8.58e-08), "const": (0, 1.51e-07, 7.33e-09)},
    "two_2x3x2136_L2_a2": {"m50": (6.98e-07, 9.55e-08, 3.8e-07), "tiny": (1.02e-07, 1.01e-07, 7.53e-09), "const": (0, 0, 0)},
    "two_2x3x2136_L3_a0": {"m50": (5.52e-07, 8.83e-08, 6.35e-07), "tiny": (1.5e-07, 1e-07, 4.05e-08), "const": (0, 7.9e-08, 2.43e-08)},
    "two_2x3x2136_L3_a1": {"m50": (2.15e-06, 5.1e-07, 7.78e-07), "tiny": (1.13e-07, 1.32e-07, 6.32e-08), "const": (0, 9.23e-08, 3.41e-08)},    # m50 out 8.6e-06
    "two_2x3x2136_L3_a2": {"m50": (7.75e-07, 1.2e-07, 1.55e-06), "tiny": (6.66e-08, 1.14e-07, 1.29e-08), "const": (0, 0, 0)},
    "small_2x3x1023_L2_a2": {"const": (0, 0, 0), "m50": (8.92e-07, 1.51e-07, 7.06e-07)},
    "small_3x5x77_L3_a1": {"pivot": (4.13e-08, 1.1e-07, 7.58e-08), "tiny": (6.14e-08, 9.65e-08, 1.31e-08), "k1000": (1.27e-05, 2.34e-06, 6.12e-06)},    # k1000 out 5.06e-05, k1000 s 2.45e-05
    "small_1x2x1_L0_a0": {"const": (0, 0, 0), "cneg": (0, 0, 0)},
    "small_1x4x10240_L0_a1": {"pivot": (5.33e-08, 1.07e-07, 1.08e-07), "tiny": (1.38e-07, 2.09e-07, 6.18e-08)},
    "small_1x4x10244_L1_a2": {"k1000": (1.6e-05, 1.66e-07, 3.39e-06), "const": (0, 0, 0), "pivot": (2.74e-08, 7.17e-08, 2.26e-08)},    # k1000 out 6.39e-05
    "two_2x3x2135_L3_a1": {"pivot": (5.69e-08, 1.53e-07, 6.35e-08), "k1000": (3.15e-05, 9.59e-06, 1.78e-05)},    # k1000 out 0.000126, k1000 dx 3.83e-05, k1000 s 7.13e-05
    "two_1x1x4100_L2_a0": {"pivot": (1.17e-08, 1.13e-07, 2.06e-07)},
    "two_1x2x1028_L0_a2": {"pivot": (4.56e-08, 9.41e-08, 3.71e-08), "tiny": (7.23e-08, 9.99e-08, 4e-08)},
    "two_4x300x8_L3_a1": {"k1000": (9.28e-05, 2.31e-05, 1.71e-05), "pivot": (1.14e-07, 7.03e-07, 1.39e-07), "m50": (4.49e-06, 1.7e-06, 6.01e-07), "tiny": (1.67e-07, 1.76e-07, 5.35e-08), "const": (0, 1.61e-07, 2.07e-08)},    # k1000 out 0.000371, k1000 dx 9.24e-05, k1000 s 6.82e-05, m50 out 1.8e-05
    "small_2x3x1024_L0_a1_g40": {"n01": (5.09e-08, 2.77e-07, 1.36e-07), "const": (0, 1.54e-07, 9.56e-09), "n31": (7.98e-08, 3.7e-07, 7.69e-08)},
    "two_2x3x2136_L0_a2_g40": {"n31": (9.68e-08, 8.11e-08, 6.05e-08), "const": (0, 0, 0), "tiny": (4.54e-08, 8.92e-08, 2.34e-08)},
    "small_2x3x1023_L1_a1_noaffine": {"pivot": (2.94e-08, 1.2e-07, 1.04e-07), "tiny": (9.43e-08, 1.53e-07, 3.34e-08)},
    "two_1x2x1028_L3_a1_noaffine_norunning": {"const": (0, 8.94e-08, 5.56e-09)},
    "small_3x5x77_L0_a2_norunning": {"m50": (1.83e-06, 9.25e-08, 4.06e-07), "const": (0, 0, 0)},    # m50 out 7.3e-06
}


def bounds(case):
    """dict out, dx, s -> [C] bound per channel"""
    hard = hard_channels(case)
    y = YARD.get(case.name, {})
    kinds = case_kinds(case)
    res = {}
    for i, (key, base) in enumerate((("out", BASE["out"]), ("dx", BASE["grad"]), ("s", BASE["grad"]))):
        b = torch.full((case.shape[1],), base, dtype=torch.float64)
        for c, k in enumerate(kinds):
            if bool(hard[c]):
                b[c] = max(base, 4.0 * y[k][i])
        res[key] = b
    return res


if __name__ == "__main__":
    for case in CASES:
        m = measure(case)
        if m:
            wide = ["%s %s %.3g" % (k, q, 4 * v[i]) for k, v in m.items() for i, (q, base) in enumerate((("out", BASE["out"]), ("dx", BASE["grad"]), ("s", BASE["grad"]))) if 4 * v[i] > base]
            print('    "%s": {%s},%s' % (case.name, ", ".join('"%s": (%.3g, %.3g, %.3g)' % ((k,) + v) for k, v in m.items()),
                                         "    # " + ", ".join(wide) if wide else ""))
