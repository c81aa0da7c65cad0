"""Test infrastructure: the cases of tests/test_splat_forms_gpu.py -- shapes, contents, references, error measure, bound -- shared with
tests/test_splat_ref_cpu.py.  No GPU in here.

Splat entries (ts_softsplat_sum_fwd, _sum_fwd_deterministic, _softmax_fwd, _sum_bwd_input, _sum_bwd_flow), one (B, C, H, W) table:
(1,1,1,1) a single pixel; (1,1,1,7) / (1,1,7,1) one row / column; (2,3,5,7) small and odd; (1,5,9,12) / (1,9,9,12) the channel counts
of the state update; (3,4,17,31) ragged, more than one block; (1,2,64,64) whole blocks; (3,2,419,418) = 525426 pixels > 524288, one
more than a grid of 2048 blocks of 256 covers: the grid-stride loops wrap, and the wrapped pixels lie in the last batch item.
Flow fields: `zero`; integer shifts `shift_pos` (+2, +1), `shift_neg` (-3, -2), `shift_out` (+W, -H: nothing arrives); `noise` (sigma
1.5); `edge`, landings uniform in [-1.5, 0.5] or [W-1.5, W+0.5] and likewise in y, so that every combination of inside flags occurs;
`collide`, every source into one 3x3 window; `absurd`, noise with a handful of pixels at +-1e9, +-3e9, 1e30, +-inf, NaN.  Metric N(0,1),
or `wide`, uniform over +-40.  Gradient outputs are noise.

ts_project_to_3d_fwd: PROJECT.  K, inv_K and T differ per batch item (blockIdx.y); depth log-uniform over 0.5..80 with a patch of zeros
and one of negative depth; motion x1 and x6 of synth.small_motion.  ts_reproject_memory_fwd: REPROJECT, the table of its docstring.

Error measure.  units = max_p |got_p - ref_p| / (EPS32 comp_p): a count of fp32 roundings, comp_p the companion of tests/splat_ref.py.
Where the companion is 0 (nothing contributes) the output has to be exactly 0.  bound = max(FLOOR, 4 x yardstick); the yardstick is the
same figure for the restatement in fp32 arithmetic against its float64 run, computed from the reference alone; FLOOR = 8: the weight
product, expf (2), v e, times w, one atomic add, the quotient's two -- so that a case whose fp32 restatement happens to be exact does
not demand bit equality; the factor 4 is block_cost_cases.bound's.

Excused pixels.  Against a mixed reference none: a pixel with D_ref = 0 is exactly zero in the kernel's output.  Against an exact
reference, and for the fused update, a pixel with D_ref = 0 is excused when some source's float64 landing lies within
1 + 4 bound EPS32 d_i of it on both axes (the fp32 position could place a vanishing weight there); so is -- the mirror image, which the
first rule leaves out -- a pixel whose D_ref is itself no larger than 4 bound EPS32 times the error scale the positions give it
(`reach`): the reference's only deposits there are vanishing weights the fp32 position may not place.  Every other pixel counts.  At
most MAX_EXCUSED = 1 % of a case's pixels may be excused; the CPU test asserts that with the fp32 restatement standing in for the kernel.
flow_mask is compared bit for bit wherever the float64 coordinate is farther from each of 0, W-1, H-1 than 4 bound times that pixel's
position scale; the same cap applies.
"""
import collections
import functools

import numpy as np
import torch

import splat_ref as ref
import synth
from splat_ref import EPS32, FIX_HALF

TS_OK, TS_ERR_NULL, TS_ERR_SHAPE, TS_ERR_UNSUPPORTED = 0, -1, -2, -3
FLOOR = 8.0
MAX_EXCUSED = 0.01
GRID_CAP_PIXELS = 2048 * 256          # grid_for: kNumCU * 8 blocks of 256
MAX_PARTS_PIXELS = 1024 * 256         # kMaxParts blocks of 256

F32, F64 = torch.float32, torch.float64


def bound(yardstick):
    return max(FLOOR, 4.0 * yardstick)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# ---- splat cases -----------------------------------------------------------------------------------------------------------------
SplatCase = collections.namedtuple("SplatCase", "name B C H W field metric")
SHIFTS = {"shift_pos": (2, 1), "shift_neg": (-3, -2), "shift_out": None}
ABSURD = (1e9, -1e9, 3e9, -3e9, 1e30, float("inf"), float("-inf"), float("nan"))
_ALL = ("zero", "shift_pos", "shift_neg", "shift_out", "noise", "edge", "collide", "absurd")
_TABLE = (((1, 1, 1, 1), ("zero", "shift_out", "noise", "edge", "absurd")),
          ((1, 1, 1, 7), ("zero", "shift_pos", "shift_neg", "noise", "edge")),
          ((1, 1, 7, 1), ("zero", "shift_pos", "shift_neg", "noise", "edge")),
          ((2, 3, 5, 7), _ALL + ("noise/wide",)),
          ((1, 5, 9, 12), ("noise", "edge", "collide")),
          ((1, 9, 9, 12), ("noise", "edge", "collide")),
          ((3, 4, 17, 31), _ALL + ("edge/wide",)),
          ((1, 2, 64, 64), ("shift_neg", "noise", "collide", "absurd")),
          ((3, 2, 419, 418), ("shift_pos", "absurd")))
SPLAT = [SplatCase("%dx%dx%dx%d_%s" % (s + (f.replace("/", "_"),)), *s, f.split("/")[0], "wide" if f.endswith("/wide") else "normal")
         for s, fields in _TABLE for f in fields]
WRAPPER_SHAPES = ((2, 3, 5, 7), (3, 4, 17, 31))


def shift_of(case):
    return SHIFTS[case.field] or (case.W, -case.H)


def flow_field(case):
    B, H, W, seed = case.B, case.H, case.W, 5200 + 7 * case.W + case.H
    if case.field == "zero":
        return torch.zeros(B, 2, H, W)
    if case.field in SHIFTS:
        f = torch.zeros(B, 2, H, W)
        f[:, 0], f[:, 1] = shift_of(case)
        return f
    if case.field in ("noise", "absurd"):
        f = _t(synth.normal(seed, "flow", (B, 2, H, W), 1.5))
        if case.field == "absurd":
            flat = f.view(B, 2, H * W)
            for k, v in enumerate(ABSURD):
                flat[(B - 1) if k % 2 else 0, (k // 2) % 2, (k * 7919 + 3) % (H * W)] = v
        return f
    xs, ys = torch.arange(W, dtype=F32).view(1, 1, W), torch.arange(H, dtype=F32).view(1, H, 1)
    if case.field == "edge":
        side = _t(synth.uniform(seed, "side", (B, 2, H, W))) < 0.5
        land = _t(synth.uniform(seed, "land", (B, 2, H, W), -1.5, 0.5))
        far = torch.tensor([W - 1.0, H - 1.0]).view(1, 2, 1, 1)
        land = torch.where(side, land, land + far + 1.0)          # [-1.5, 0.5] | [n - 1.5, n + 0.5]
    else:                                                          # collide: landings in [c, c + 2) on both axes
        assert case.field == "collide"
        land = _t(synth.uniform(seed, "land", (B, 2, H, W), 0.0, 1.999))
        land = land + torch.tensor([float(max(0, W // 2 - 1)), float(max(0, H // 2 - 1))]).view(1, 2, 1, 1)
    return torch.stack([land[:, 0] - xs, land[:, 1] - ys], 1).contiguous()


@functools.lru_cache(maxsize=4)
def splat_inputs(case):
    """fp32: input, flow, metric, grad_out (shared: read only)"""
    B, C, H, W, seed = case.B, case.C, case.H, case.W, 5100 + 13 * case.W + case.C
    metric = _t(synth.normal(seed, "metric", (B, 1, H, W))) if case.metric == "normal" else _t(synth.uniform(seed, "metric", (B, 1, H, W), -40.0, 40.0))
    return _t(synth.normal(seed, "in", (B, C, H, W))), flow_field(case), metric, _t(synth.normal(seed, "gout", (B, C, H, W)))


# one reference of one quantity: the Splat (out, comp, den, count, reach) and, for an exact reference, the float64 landings with their
# companions (None: mixed, nothing is excused)
Ref = collections.namedtuple("Ref", "splat ox oy dx dy")


def _ref(inp, flow, metric, mode, pos_dtype):
    s, _ = ref.splat_reference(inp, flow, metric, mode, pos_dtype)
    if pos_dtype is not None:
        return Ref(s, None, None, None, None)
    ox, oy, _ = ref.positions(flow)
    dx, dy = ref.position_companions(flow)
    return Ref(s, ox, oy, dx, dy)


@functools.lru_cache(maxsize=4)
def splat_reference(case):
    """-> {"summation" | "softmax": {"mixed": Ref, "exact": Ref, "fp32": the restatement's fp32 output}}"""
    inp, flow, metric, _ = splat_inputs(case)
    out = {}
    for mode in ("summation", "softmax"):
        m64 = metric.double() if mode == "softmax" else None
        out[mode] = {"mixed": _ref(inp.double(), flow.double(), m64, mode, F32), "exact": _ref(inp.double(), flow.double(), m64, mode, None),
                     "fp32": ref.splat_reference(inp, flow, metric if mode == "softmax" else None, mode)[0].out}
    return out


@functools.lru_cache(maxsize=4)
def grad_reference(case):
    """-> (grad_input, companion, grad_flow, companion) of the mixed reference, and (grad_input, grad_flow) of the fp32 restatement"""
    inp, flow, _, gout = splat_inputs(case)
    g32 = ref.sum_grads(inp, flow, gout)
    return ref.sum_grads(inp.double(), flow.double(), gout.double(), F32), (g32[0], g32[2])


# ---- error measure ---------------------------------------------------------------------------------------------------------------
def units(got, want, comp, extra=None, skip=None):
    """max |got - want| / (EPS32 comp [+ extra]); an element whose scale is 0 has to be exactly `want`; non-finite -> inf"""
    scale = EPS32 * comp.double() + (0.0 if extra is None else extra)
    d = (got.double() - want.double()).abs()
    u = torch.where(scale > 0, d / scale, torch.where(d == 0, torch.zeros_like(d), torch.full_like(d, float("inf"))))
    u = torch.nan_to_num(u, nan=float("inf"), posinf=float("inf"))
    if skip is not None:
        u = torch.where(skip.expand_as(u), torch.zeros_like(u), u)
    return float(u.max()) if u.numel() else 0.0


def excused(R, bnd):
    """pixels [B, 1, H, W] of an exact reference that the fp32 position may fill or leave differently (the module's docstring)"""
    s = R.splat
    B, _, H, W = s.count.shape
    if R.ox is None:
        return torch.zeros(B, 1, H, W, dtype=torch.bool)
    slack = 4.0 * bnd * EPS32
    near = ref.near_landings(R.ox, R.oy, (slack * R.dx).clamp(max=0.5), (slack * R.dy).clamp(max=0.5), H, W).unsqueeze(1)
    out = (s.count == 0) & near
    if s.den is not None:
        out = out | ((s.count > 0) & (s.den - 1e-22 <= slack * s.reach))
    return out


def splat_units(got, R, bnd, extra=None):
    """-> (units, share of excused pixels) of a splat output against a Ref, excusing at the bound `bnd`"""
    ex = excused(R, bnd)
    return units(got, R.splat.out, R.splat.comp, extra, ex), float(ex.double().mean())


def judge(got, fp32, R, extra=None):
    """-> (units of `got`, yardstick, bound, excused share): the yardstick is the fp32 restatement against the same Ref, excusing at FLOOR"""
    yard, _ = splat_units(fp32, R, FLOOR, extra)
    b = bound(yard)
    u, share = splat_units(got, R, b, extra)
    return u, yard, b, share


# ---- ts_project_to_3d_fwd --------------------------------------------------------------------------------------------------------
ProjectCase = collections.namedtuple("ProjectCase", "name B C H W k_dim inv_k_dim eps motion")


def _pcase(B, C, H, W, kd, ikd, eps, motion):
    return ProjectCase("%dx%dx%dx%d_k%d_ik%d_eps%g_x%d" % (B, C, H, W, kd, ikd, eps, motion), B, C, H, W, kd, ikd, eps, motion)


PROJECT = [_pcase(2, 3, 5, 7, kd, ikd, eps, mo) for kd in (3, 4) for ikd in (3, 4) for eps in (1e-7, 1e-3) for mo in (1, 6)]
PROJECT += [_pcase(1, 1, 1, 1, 4, 4, 1e-7, 1), _pcase(1, 1, 1, 1, 3, 4, 1e-3, 6), _pcase(1, 5, 17, 31, 4, 3, 1e-7, 1), _pcase(1, 5, 17, 31, 3, 3, 1e-3, 6),
            _pcase(3, 1, 9, 12, 3, 4, 1e-7, 6), _pcase(3, 1, 9, 12, 4, 4, 1e-3, 1), _pcase(1, 2, 600, 438, 4, 3, 1e-7, 6)]


def pinhole(B, H, W, scale=1.0):
    """[B, 4, 4] fp32, a different focal length and principal point per batch item"""
    K = np.zeros((B, 4, 4), dtype=np.float64)
    for b in range(B):
        f = max(W, H, 2) * (1.0 + 0.15 * b) * scale
        K[b] = np.array([[f, 0, (W - 1) / 2.0 + 0.3 * b, 0], [0, f * 1.02, (H - 1) / 2.0 - 0.2 * b, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    return K.astype(np.float32)


@functools.lru_cache(maxsize=4)
def project_inputs(case):
    """fp32: depth, K [B, k_dim, k_dim], inv_K [B, inv_k_dim, inv_k_dim], T"""
    B, C, H, W = case.B, case.C, case.H, case.W
    seed = 5300 + 11 * W + H
    depth = torch.exp(_t(synth.uniform(seed, "depth", (B, C, H, W), float(np.log(0.5)), float(np.log(80.0)))))
    depth[:, :, H // 3:H // 3 + max(1, H // 5), W // 4:W // 4 + max(1, W // 5)] = 0.0
    if H > 1 and W > 1:
        depth[:, :, H // 2:H // 2 + max(1, H // 6), W // 2:W // 2 + max(1, W // 6)] *= -1.0
    K = pinhole(B, H, W)
    inv = np.linalg.inv(K.astype(np.float64)).astype(np.float32)
    T = synth.small_motion(seed, B, max_deg=1.0 * case.motion, max_t=0.1 * case.motion)
    return depth, _t(K[:, :case.k_dim, :case.k_dim]), _t(inv[:, :case.inv_k_dim, :case.inv_k_dim]), _t(T)


@functools.lru_cache(maxsize=4)
def project_reference(case):
    """-> (float64 Projected, fp32 Projected)"""
    ins = project_inputs(case)
    return ref.project(*[t.double() for t in ins], eps=case.eps), ref.project(*ins, eps=case.eps)


def mask_strict(p64, bnd, H, W):
    """where flow_mask is compared bit for bit: the float64 coordinate farther from 0, W-1, H-1 than 4 bound times its position scale"""
    mx, my = 4.0 * bnd * EPS32 * p64.a_sx, 4.0 * bnd * EPS32 * p64.a_sy
    return ((p64.sx.abs() > mx) & ((p64.sx - (W - 1)).abs() > mx) & (p64.sy.abs() > my) & ((p64.sy - (H - 1)).abs() > my)
            & torch.isfinite(mx) & torch.isfinite(my))


def judge_project(got_tri, got_flow, got_mask, case):
    """-> {"tri" | "flow": (units, yardstick, bound), "mask": (mismatches where strict, share not strict)}; a None output is left out"""
    p64, p32 = project_reference(case)
    out = {}
    yf = units(p32.flow, p64.flow, p64.a_flow)
    if got_tri is not None:
        y = units(p32.tri, p64.tri, p64.a_tri)
        out["tri"] = (units(got_tri, p64.tri, p64.a_tri), y, bound(y))
    if got_flow is not None:
        out["flow"] = (units(got_flow, p64.flow, p64.a_flow), yf, bound(yf))
    if got_mask is not None:
        strict = mask_strict(p64, bound(yf), case.H, case.W)
        out["mask"] = (int(((got_mask.bool() != p64.mask) & strict).sum()), float((~strict).double().mean()))
    return out


# ---- ts_reproject_memory_fwd -----------------------------------------------------------------------------------------------------
ReprojCase = collections.namedtuple("ReprojCase", "name B Hf Wf h w k n_in n_out pose k_dim per_item_baseline gap")
REPROJECT = [ReprojCase("1x8x8_to_1x1_local", 1, 8, 8, 1, 1, 1, 0, 1, "identity", 4, False, 0),                 # sh = sw = 0
             ReprojCase("1x9x17_to_1x2_memory", 1, 9, 17, 1, 2, 1, 0, 0, "small", 4, False, 0),                  # memory only
             ReprojCase("2x43x61_to_5x7_first", 2, 43, 61, 5, 7, 0, 0, 1, "x6", 4, False, 0),                    # first frame: local map from the disparity alone
             ReprojCase("2x75x109_to_9x13", 2, 75, 109, 9, 13, 2, 2, 3, "small", 4, False, 0),                   # small ragged shape
             ReprojCase("3x139x251_to_17x31_crop", 3, 139, 251, 17, 31, 3, 3, 2, "composed", 3, True, 5),        # cropping, k_dim 3, T_b, baseline_ptr, strided
             ReprojCase("2x9x13_same_grid", 2, 9, 13, 9, 13, 1, 1, 2, "small", 4, False, 0),                        # the resize is the identity
             ReprojCase("5x300x310_to_230x230", 5, 300, 310, 230, 230, 1, 0, 1, "small", 4, False, 0)]           # 264500 > 262144: nparts capped, every loop wraps
BASELINE = 0.54


@functools.lru_cache(maxsize=2)
def reproject_inputs(case):
    """fp32 dict: prev_disp [B, 1, Hf, Wf] (2..60 with a patch of exact zeros), mem_disp, mem_cost, local_map (None where the case has
    none), K, T_a, T_b (None unless composed), baseline [B], factor"""
    c = case
    seed = 5400 + 3 * c.Wf + c.h
    disp = _t(synth.smooth(synth.uniform(seed, "disp", (c.B, 1, c.Hf, c.Wf), 2.0, 60.0), 1)).clamp(2.0, 60.0)
    disp[:, :, c.Hf // 4:c.Hf // 4 + max(1, c.Hf // 6), c.Wf // 3:c.Wf // 3 + max(1, c.Wf // 6)] = 0.0
    top = 60.0 * c.w / c.Wf
    plane = lambda tag, n: _t(synth.uniform(seed, tag, (c.B, n, c.h, c.w), 0.03 * top, top)) if n else None
    eye = torch.eye(4).unsqueeze(0).repeat(c.B, 1, 1)
    T_b = None
    if c.pose == "identity":
        T_a = eye
    elif c.pose == "composed":
        T_a, T_b = _t(synth.small_motion(seed, c.B)), _t(synth.small_motion(seed + 1, c.B, max_deg=2.0, max_t=0.2))
    else:
        m = 6.0 if c.pose == "x6" else 1.0
        T_a = _t(synth.small_motion(seed, c.B, max_deg=m, max_t=0.1 * m))
    base = torch.tensor([BASELINE * (1.0 + 0.25 * b) for b in range(c.B)]) if c.per_item_baseline else torch.full((c.B,), BASELINE)
    return dict(prev_disp=disp, mem_disp=plane("mem", c.k), mem_cost=None if not c.k else _t(synth.normal(seed, "cost", (c.B, c.k, c.h, c.w))),
                local_map=plane("local", c.n_in), K=_t(pinhole(c.B, c.Hf, c.Wf)[:, :c.k_dim, :c.k_dim]), T_a=T_a, T_b=T_b, baseline=base,
                factor=float(c.Wf) / c.w)


def _reproject(ins, case, dt):
    to = lambda t: None if t is None else t.to(dt)
    return ref.reproject(to(ins["prev_disp"]), to(ins["mem_disp"]), to(ins["mem_cost"]), to(ins["local_map"]), case.n_out, to(ins["K"]),
                         to(ins["T_a"]), to(ins["T_b"]), to(ins["baseline"]), ins["factor"], case.h, case.w)


@functools.lru_cache(maxsize=2)
def reproject_reference(case):
    """-> (float64 Moved, Ref of all its planes, fp32 Moved)"""
    ins = reproject_inputs(case)
    m64, m32 = _reproject(ins, case, F64), _reproject(ins, case, F32)
    return m64, Ref(m64.splat, m64.ox, m64.oy, m64.dx, m64.dy), m32


def split_planes(x, k, n_out):
    """[B, 2k + n_out, h, w] -> (disp, cost, local)"""
    return x[:, :k], x[:, k:2 * k], x[:, 2 * k:2 * k + n_out]
