"""Test infrastructure: a plain restatement of the temporal warp (K2: csrc/softsplat.hip, csrc/reproject.hip, csrc/project.hpp), tap by
tap, in the dtype of its inputs, with an error scale ("companion") for everything it returns.  No GPU in here.

Splat.  Every source pixel has four taps -- column, row, weight, inside flag -- which are scatter-added (oracle/splat.py;
softsplat.py:14-52 of the reference).  A source none of whose taps is inside the frame is DROPPED: it deposits nothing and has zero
gradient with respect to input, flow and metric.  That covers flows of +-1e9, +-3e9 (beyond int), 1e30, +-inf and NaN: `footprint`
masks such pixels before any arithmetic, so no inf - inf or 0 * NaN is ever formed.  The normalised modes (average, linear, softmax)
are N / (D + 1e-22) as in FunctionSoftsplat (softsplat.py:334-360).

The position has a dtype of its own, as in tests/block_cost_ref.py.  `ox = x + flow` is one fp32 add in every kernel that takes the
flow as an input, and contraction cannot change a lone add.  On float64 inputs:
  exact   pos_dtype = float64: everything in float64;
  mixed   pos_dtype = float32: ox, oy from that fp32 add, everything after it in float64.  The tap a gradient belongs to is then the
          kernel's by construction, at integer landings too (floor gives the right-hand derivative in both).
Gradients are autograd of the mixed reference.

Companions.  The error scale of a quantity is the same expression with every product replaced by its absolute value, in units of one
fp32 rounding (multiply by EPS32); through a division it propagates as (A_num + |q| A_den) / |den|.  For a normalised splat at pixel p
with contributors i, weights w_i, e_i = exp(metric_i) (or the metric, or 1) and values v_i whose own companions are a_i >= |v_i|:
    comp_p = A_p / D_p + |out_p| + M_p / D_p + G_p / D_p,        D_p including the 1e-22,
    A_p = sum w_i e_i a_i,   M_p = sum w_i e_i |v_i - out_p| m_i,   G_p = sum e_i |v_i - out_p| (|dw/dox| dx_i + |dw/doy| dy_i),
m_i being the relative error scale of e_i (1 + |metric_i| for exp) and (dx_i, dy_i) the position's own companion: 0 in the mixed
reference of a flow-input entry, |x| + |flow| per axis in its exact reference, the projection's for the fused update.  Plain
summation: comp_p = A_p + G_p with |v_i| in G.  The deterministic entry adds n_p 2^-41 absolute, n_p deposits on p each rounded to the
2^-40 grid of kFix (`FIX_HALF`).  Gradients: the same construction over their four-tap sums (`sum_grads`, `softsplat_grads`).

project / reproject restate ts::project_pixel and the fused kernels' own algebra per plane (bf = baseline K00 / factor, one flow and
one metric shared by all planes, [pd | local_map] cropped to n_local_out); in float64 they equal oracle.geometry.project_to_3d and
oracle.temporal.update_past_cost / update_local_map, which tests/test_splat_ref_cpu.py pins.
"""
import collections

import torch

EPS32 = 2.0 ** -23          # torch.finfo(torch.float32).eps
FIX_HALF = 2.0 ** -41       # half a step of the deterministic entry's fixed point
MODES = ("summation", "average", "linear", "softmax")

Foot = collections.namedtuple("Foot", "alive lin w dwx dwy ins ox oy")


def positions(flow, pos_dtype=None):
    """flow [B, 2, H, W] -> (ox, oy) [B, H, W] in flow.dtype: the value of `x + flow` computed in pos_dtype, the derivative 1.  Pixels
    that `footprint` will drop keep their (possibly non-finite) value here; it masks them."""
    B, _, H, W = flow.shape
    dt, pdt = flow.dtype, pos_dtype or flow.dtype
    f = flow.detach().to(pdt)
    ox = (torch.arange(W, dtype=pdt).view(1, 1, W) + f[:, 0]).to(dt)
    oy = (torch.arange(H, dtype=pdt).view(1, H, 1) + f[:, 1]).to(dt)
    return ox, oy, flow


def footprint(ox, oy, H, W, carrier=None):
    """positions [B, H, W] -> Foot.  `carrier` [B, 2, h, w]: the tensor the positions' derivative is 1 of (the flow), or None when ox, oy
    carry their own graph.  Dropped pixels are masked before any arithmetic."""
    B = ox.shape[0]
    dt = ox.dtype
    with torch.no_grad():
        x0, y0 = torch.floor(ox.detach()), torch.floor(oy.detach())
        xa, xb = (x0 >= 0) & (x0 < W), (x0 + 1 >= 0) & (x0 + 1 < W)
        ya, yb = (y0 >= 0) & (y0 < H), (y0 + 1 >= 0) & (y0 + 1 < H)
        alive = (xa | xb) & (ya | yb)
        x0, y0 = torch.where(alive, x0, torch.zeros_like(x0)), torch.where(alive, y0, torch.zeros_like(y0))
    zero = torch.zeros((), dtype=dt)
    ox, oy = torch.where(alive, ox, zero), torch.where(alive, oy, zero)
    if carrier is not None and carrier.requires_grad:
        c = torch.where(alive.unsqueeze(1), carrier, zero)
        ox, oy = ox.detach() + (c[:, 0] - c[:, 0].detach()), oy.detach() + (c[:, 1] - c[:, 1].detach())
    ax, ay = ox - x0, oy - y0
    flat = lambda t: t.reshape(B, H * W)
    ins = [flat(m & alive) for m in (xa & ya, xb & ya, xa & yb, xb & yb)]
    gate = [m.to(dt) for m in ins]
    w = [flat((1 - ax) * (1 - ay)) * gate[0], flat(ax * (1 - ay)) * gate[1], flat((1 - ax) * ay) * gate[2], flat(ax * ay) * gate[3]]
    dwx = [flat(-(1 - ay)) * gate[0], flat(1 - ay) * gate[1], flat(-ay) * gate[2], flat(ay) * gate[3]]
    dwy = [flat(-(1 - ax)) * gate[0], flat(-ax) * gate[1], flat(1 - ax) * gate[2], flat(ax) * gate[3]]
    lin = [flat(((y0 + dy).clamp(0, H - 1) * W + (x0 + dx).clamp(0, W - 1)).long()) for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1))]
    return Foot(alive, lin, w, dwx, dwy, ins, ox, oy)


def deposit(foot, src, weights=None):
    """sum over the four taps of src [B, C, HW] * weights[tap] [B, HW] or [B, C, HW], scattered to the taps' pixels -> [B, C, HW]"""
    out = None
    for t in range(4):
        wt = (foot.w if weights is None else weights)[t]
        term = src * (wt.unsqueeze(1) if wt.dim() == 2 else wt)
        if out is None:
            out = torch.zeros_like(term)
        out = out.scatter_add(2, foot.lin[t].unsqueeze(1).expand_as(term), term)
    return out


def near_landings(ox, oy, sx, sy, H, W):
    """pixels within 1 + sx of a source's landing ox along x and 1 + sy of oy along y (sx, sy < 1) -> bool [B, H, W]: where a position
    off by its own error scale could place a vanishing weight.  Sources outside the frame count; non-finite ones do not."""
    B = ox.shape[0]
    ok = torch.isfinite(ox) & torch.isfinite(oy) & (ox > -3) & (ox < W + 2) & (oy > -3) & (oy < H + 2)
    zero = torch.zeros_like(ox)
    ox, oy = torch.where(ok, ox, zero), torch.where(ok, oy, zero)
    x0, y0 = torch.floor(ox), torch.floor(oy)
    near = torch.zeros(B, H * W, dtype=torch.bool)
    for dy in (-1, 0, 1, 2):
        for dx in (-1, 0, 1, 2):
            px, py = x0 + dx, y0 + dy
            hit = ok & ((px - ox).abs() < 1 + sx) & ((py - oy).abs() < 1 + sy) & (px >= 0) & (px < W) & (py >= 0) & (py < H)
            lin = (py.clamp(0, H - 1) * W + px.clamp(0, W - 1)).long().reshape(B, H * W)
            near = near | torch.zeros(B, H * W, dtype=torch.int32).scatter_add(1, lin, hit.reshape(B, H * W).to(torch.int32)).bool()
    return near.reshape(B, H, W)


def collect(foot, field, weights=None):
    """the adjoint of `deposit`: per source, sum over the taps of field[tap's pixel] * weights[tap]"""
    B, C, HW = field.shape
    out = torch.zeros(B, C, HW, dtype=field.dtype)
    for t in range(4):
        out = out + torch.gather(field, 2, foot.lin[t].unsqueeze(1).expand(B, C, HW)) * (foot.w if weights is None else weights)[t].unsqueeze(1)
    return out


def _weigh(inp, metric, mode):
    """-> (x [B, C, H, W] the splatted numerator's values, e [B, 1, H, W] or None, m the relative error scale of e)"""
    if mode == "summation":
        return inp, None, None
    if mode == "average":
        return inp, torch.ones_like(inp[:, :1]), torch.zeros_like(inp[:, :1])
    if mode == "linear":
        return inp, metric, torch.ones_like(metric)
    if mode == "softmax":
        return inp, metric.exp(), 1 + metric.detach().abs()
    raise ValueError("unknown splat type " + str(mode))


def splat_sum(inp, flow, pos_dtype=None):
    """ts_softsplat_sum_fwd: differentiable with respect to inp and flow"""
    B, C, H, W = inp.shape
    ox, oy, carrier = positions(flow, pos_dtype)
    return deposit(footprint(ox, oy, H, W, carrier), inp.reshape(B, C, H * W)).reshape(B, C, H, W)


def softsplat(inp, flow, metric, mode, pos_dtype=None):
    """FunctionSoftsplat in all four modes: differentiable with respect to inp, flow and metric"""
    B, C, H, W = inp.shape
    x, e, _ = _weigh(inp, metric, mode)
    ox, oy, carrier = positions(flow, pos_dtype)
    foot = footprint(ox, oy, H, W, carrier)
    if e is None:
        return deposit(foot, x.reshape(B, C, H * W)).reshape(B, C, H, W)
    e = e.reshape(B, 1, H * W)
    num, den = deposit(foot, x.reshape(B, C, H * W) * e), deposit(foot, e)
    return (num / (den + 1e-22)).reshape(B, C, H, W)


Splat = collections.namedtuple("Splat", "out comp den count reach")


def splat_companions(foot, v, e=None, m=None, a=None, dx=None, dy=None):
    """v [B, C, H, W] on the footprint `foot`; e, m [B, 1, H, W] (None: plain summation); a the values' own companions (None: |v|);
    dx, dy [B, H, W] the position's companions (None: 0) -> Splat: out, its companion (units of EPS32), D (None for summation), the
    number of deposits per pixel, and `reach`, the error scale of D itself from the positions (for the excused pixels)"""
    B, C, H, W = v.shape
    HW = H * W
    with torch.no_grad():
        v = v.reshape(B, C, HW)
        a = v.abs() if a is None else a.reshape(B, C, HW)
        one = torch.ones(B, 1, HW, dtype=v.dtype)
        count = deposit(foot, one, [(i & (wt > 0)).to(v.dtype) for i, wt in zip(foot.ins, foot.w)])     # deposits of a non-zero weight
        slope = None
        if dx is not None:
            slope = [foot.dwx[t].abs() * dx.reshape(B, HW) + foot.dwy[t].abs() * dy.reshape(B, HW) for t in range(4)]
        if e is None:
            out = deposit(foot, v)
            comp = deposit(foot, a)
            if slope is not None:
                comp = comp + deposit(foot, v.abs(), slope)
            shape = lambda t: t.reshape(B, -1, H, W)
            return Splat(shape(out), shape(comp), None, shape(count), shape(deposit(foot, one, slope)) if slope is not None else None)
        e, m = e.reshape(B, 1, HW), m.reshape(B, 1, HW)
        den = deposit(foot, e) + 1e-22
        out = deposit(foot, v * e) / den
        spread = [(v - torch.gather(out, 2, foot.lin[t].unsqueeze(1).expand(B, C, HW))).abs() for t in range(4)]
        comp = deposit(foot, a * e) / den + out.abs()
        comp = comp + deposit(foot, e * m, [spread[t] * foot.w[t].unsqueeze(1) for t in range(4)]) / den
        reach = None
        if slope is not None:
            comp = comp + deposit(foot, e, [spread[t] * slope[t].unsqueeze(1) for t in range(4)]) / den
            reach = deposit(foot, e.abs(), slope)
        shape = lambda t: None if t is None else t.reshape(B, -1, H, W)
        return Splat(shape(out), shape(comp), shape(den), shape(count), shape(reach))


def position_companions(flow):
    """|x| + |flow| per axis -> dx, dy [B, H, W]; 0 where the fp32 add is exact (integer shifts: nothing was rounded) and where the
    value is not finite (such pixels are dropped)"""
    B, _, H, W = flow.shape
    f = torch.where(torch.isfinite(flow), flow.abs(), torch.zeros_like(flow))
    dx, dy = torch.arange(W, dtype=flow.dtype).view(1, 1, W) + f[:, 0], torch.arange(H, dtype=flow.dtype).view(1, H, 1) + f[:, 1]
    (ox, oy, _), (ox32, oy32, _) = positions(flow.double()), positions(flow.double(), torch.float32)
    return torch.where(ox == ox32, torch.zeros_like(dx), dx), torch.where(oy == oy32, torch.zeros_like(dy), dy)


def splat_reference(inp, flow, metric, mode, pos_dtype=None):
    """-> Splat of one FunctionSoftsplat mode on float64 (or, for the yardstick, fp32) inputs.  pos_dtype = float32 on float64 inputs is
    the mixed reference (position companions 0), pos_dtype None the exact one (|x| + |flow|)."""
    B, C, H, W = inp.shape
    with torch.no_grad():
        x, e, m = _weigh(inp, metric, mode)
        ox, oy, _ = positions(flow, pos_dtype)
        foot = footprint(ox, oy, H, W)
        dx, dy = (None, None) if pos_dtype == torch.float32 and inp.dtype == torch.float64 else position_companions(flow)
        return splat_companions(foot, x, e, m, None, dx, dy), foot


def sum_grads(inp, flow, gout, pos_dtype=None):
    """ts_softsplat_sum_bwd_input / _bwd_flow written out: -> (grad_input, its companion, grad_flow, its companion); the values are
    what autograd of `splat_sum` gives (tests/test_splat_ref_cpu.py pins that)"""
    B, C, H, W = inp.shape
    HW = H * W
    with torch.no_grad():
        ox, oy, _ = positions(flow, pos_dtype)
        foot = footprint(ox, oy, H, W)
        g, v = gout.reshape(B, C, HW), inp.reshape(B, C, HW)
        gi, ci = collect(foot, g), collect(foot, g.abs())
        gf = torch.stack([(v * collect(foot, g, d)).sum(1) for d in (foot.dwx, foot.dwy)], 1)
        cf = torch.stack([(v.abs() * collect(foot, g.abs(), [t.abs() for t in d])).sum(1) for d in (foot.dwx, foot.dwy)], 1)
        return gi.reshape(B, C, H, W), ci.reshape(B, C, H, W), gf.reshape(B, 2, H, W), cf.reshape(B, 2, H, W)


def softsplat_grads(inp, flow, metric, mode, gout, pos_dtype=None):
    """The backward of FunctionSoftsplat stage by stage (quotient, four-tap sums, weighting), every stage with its companion ->
    {"input" | "flow" | "metric": (gradient, companion)}; the values are what autograd of `softsplat` gives."""
    B, C, H, W = inp.shape
    HW = H * W
    if mode == "summation":
        gi, ci, gf, cf = sum_grads(inp, flow, gout, pos_dtype)
        return {"input": (gi, ci), "flow": (gf, cf)}
    with torch.no_grad():
        x, e, _ = _weigh(inp, metric, mode)
        ox, oy, _ = positions(flow, pos_dtype)
        foot = footprint(ox, oy, H, W)
        x, e, g = x.reshape(B, C, HW), e.reshape(B, 1, HW), gout.reshape(B, C, HW)
        den = deposit(foot, e) + 1e-22
        out, aout = deposit(foot, x * e) / den, deposit(foot, x.abs() * e) / den
        gn, cn = g / den, g.abs() / den                                              # d out / d N
        gd, cd = -(g * out).sum(1, keepdim=True) / den, (g.abs() * aout).sum(1, keepdim=True) / den     # d out / d D
        gxe, cxe = collect(foot, gn), collect(foot, cn)                              # with respect to x * e
        ged, ced = collect(foot, gd), collect(foot, cd)                              # with respect to e, through D
        ge, ce = (gxe * x).sum(1, keepdim=True) + ged, (cxe * x.abs()).sum(1, keepdim=True) + ced
        res = {"input": ((gxe * e).reshape(B, C, H, W), (cxe * e.abs()).reshape(B, C, H, W))}
        gf, cf = [], []
        for d in (foot.dwx, foot.dwy):
            ad = [t.abs() for t in d]
            gf.append((x * e * collect(foot, gn, d)).sum(1) + (e * collect(foot, gd, d)).sum(1))
            cf.append(((x * e).abs() * collect(foot, cn, ad)).sum(1) + (e.abs() * collect(foot, cd, ad)).sum(1))
        res["flow"] = (torch.stack(gf, 1).reshape(B, 2, H, W), torch.stack(cf, 1).reshape(B, 2, H, W))
        if mode == "linear":
            res["metric"] = (ge.reshape(B, 1, H, W), ce.reshape(B, 1, H, W))
        elif mode == "softmax":
            res["metric"] = ((ge * e).reshape(B, 1, H, W), (ce * e).reshape(B, 1, H, W))
        return res


# ---- rigid re-projection ---------------------------------------------------------------------------------------------------------
def _pad4(K):
    if K.shape[-1] == 4:
        return K
    K4 = torch.eye(4, dtype=K.dtype).unsqueeze(0).repeat(K.shape[0], 1, 1)
    K4[:, :3, :3] = K
    return K4


def _rays(iK, H, W):
    """iK [B, 3, 3] -> r = iK [u v 1]^T and its companion, [B, 3, 1, H, W]"""
    dt = iK.dtype
    u = torch.arange(W, dtype=dt).view(1, 1, 1, 1, W)
    v = torch.arange(H, dtype=dt).view(1, 1, 1, H, 1)
    col = lambda M, j: M[:, :, j].reshape(-1, 3, 1, 1, 1)
    return col(iK, 0) * u + col(iK, 1) * v + col(iK, 2), col(iK.abs(), 0) * u + col(iK.abs(), 1) * v + col(iK.abs(), 2)


def _move(P, AP, r, Ar, z, az=None):
    """P, AP [B, 3, 4]; r, Ar [B, 3, 1, H, W]; z [B, C, H, W], az its companion (None: |z|) -> cam [B, 3, C, H, W] = P [r z; 1] and its
    companion"""
    X, AX = r * z.unsqueeze(1), Ar * (z.abs() if az is None else az).unsqueeze(1)
    el = lambda M, i, j: M[:, i, j].reshape(-1, 1, 1, 1)
    cam = torch.stack([el(P, i, 0) * X[:, 0] + el(P, i, 1) * X[:, 1] + el(P, i, 2) * X[:, 2] + el(P, i, 3) for i in range(3)], 1)
    acam = torch.stack([el(AP, i, 0) * AX[:, 0] + el(AP, i, 1) * AX[:, 1] + el(AP, i, 2) * AX[:, 2] + el(AP, i, 3) for i in range(3)], 1)
    return cam, acam


Projected = collections.namedtuple("Projected", "tri flow mask sx sy a_tri a_sx a_sy a_flow")


def project(depth, K, inv_K, T, eps=1e-7):
    """ts_project_to_3d_fwd (ts::project_pixel): depth [B, C, H, W], K / inv_K [B, 3|4, 3|4], T [B, 4, 4] -> Projected: triangular depth,
    flow [B, 2C, H, W] (x, y interleaved per plane), mask, the source coordinates and every companion (units of EPS32)"""
    B, C, H, W = depth.shape
    dt = depth.dtype
    with torch.no_grad():
        K4 = _pad4(K)
        P, AP = torch.matmul(K4, T)[:, :3], torch.matmul(K4.abs(), T.abs())[:, :3]
        r, Ar = _rays(inv_K[:, :3, :3], H, W)
        cam, acam = _move(P, AP, r, Ar, depth)
        den = cam[:, 2] + eps
        aden = acam[:, 2] + abs(eps)
        sx, sy = cam[:, 0] / den, cam[:, 1] / den
        a_sx = (acam[:, 0] + sx.abs() * aden) / den.abs() + sx.abs()
        a_sy = (acam[:, 1] + sy.abs() * aden) / den.abs() + sy.abs()
        u = torch.arange(W, dtype=dt).view(1, 1, 1, W)
        v = torch.arange(H, dtype=dt).view(1, 1, H, 1)
        flow = torch.stack([sx - u, sy - v], 2)
        a_flow = torch.stack([a_sx + (sx - u).abs(), a_sy + (sy - v).abs()], 2)
        mask = (sx >= 0) & (sx <= W - 1) & (sy >= 0) & (sy <= H - 1)
        return Projected(cam[:, 2], flow.reshape(B, 2 * C, H, W), mask, sx, sy, acam[:, 2], a_sx, a_sy, a_flow.reshape(B, 2 * C, H, W))


# ---- the fused state update ------------------------------------------------------------------------------------------------------
def resize_disparity(prev_disp, h, w):
    """reproject_prepare: prev_disp [B, 1, Hf, Wf] -> [B, 1, h, w], align-corners bilinear of disp * w / Wf, written per tap (a target
    axis of size 1: scale 0, both taps on cell 0), and its companion: the taps' absolute sum plus what one rounding of the source
    coordinates sy, sx moves the result by (|sy| |bot - top| and likewise along x: a fraction next to 0 has no relative accuracy)"""
    B, _, Hf, Wf = prev_disp.shape
    dt = prev_disp.dtype

    def axis(n_in, n_out):
        scale = torch.tensor(float(n_in - 1), dtype=dt) / torch.tensor(float(n_out - 1), dtype=dt) if n_out > 1 else torch.tensor(0.0, dtype=dt)
        s = scale * torch.arange(n_out, dtype=dt)
        i0 = s.to(torch.int64)
        i1 = i0 + (i0 < n_in - 1).to(torch.int64)
        return i0, i1, s - i0.to(dt), s
    y0, y1, ly, sy = axis(Hf, h)
    x0, x1, lx, sx = axis(Wf, w)
    s = prev_disp[:, 0] * torch.tensor(float(w), dtype=dt) / torch.tensor(float(Wf), dtype=dt)
    at = lambda yi, xi: s[:, yi][:, :, xi]
    lx, ly = lx.view(1, 1, w), ly.view(1, h, 1)
    top = (1 - lx) * at(y0, x0) + lx * at(y0, x1)
    bot = (1 - lx) * at(y1, x0) + lx * at(y1, x1)
    a = s.abs()
    aat = lambda yi, xi: a[:, yi][:, :, xi]
    comp = (1 - ly) * ((1 - lx) * aat(y0, x0) + lx * aat(y0, x1)) + ly * ((1 - lx) * aat(y1, x0) + lx * aat(y1, x1))
    # a fraction that one rounding of the coordinate could have taken from the end of the cell before: that cell's slope counts too
    yp, xp = (y0 - 1).clamp(min=0), (x0 - 1).clamp(min=0)
    edge_y, edge_x = (ly <= 4 * EPS32 * sy.view(1, h, 1)).to(dt), (lx <= 4 * EPS32 * sx.view(1, 1, w)).to(dt)
    row = lambda yi: (1 - lx) * at(yi, x0) + lx * at(yi, x1)
    col = lambda xi: (1 - ly) * at(y0, xi) + ly * at(y1, xi)
    comp = comp + sy.view(1, h, 1) * torch.maximum((bot - top).abs(), edge_y * (top - row(yp)).abs())
    comp = comp + sx.view(1, 1, w) * torch.maximum((col(x1) - col(x0)).abs(), edge_x * (col(x0) - col(xp)).abs())
    return ((1 - ly) * top + ly * bot).unsqueeze(1), comp.unsqueeze(1)


Moved = collections.namedtuple("Moved", "pd disp cost local splat foot k n_out ox oy dx dy")


def reproject(prev_disp, mem_disp, mem_cost, local_map, n_local_out, K, T_a, T_b, baseline, factor, h, w):
    """ts_reproject_memory_fwd, plane by plane.  mem_disp / mem_cost [B, k, h, w] or None; local_map [B, n, h, w] or None; baseline a
    tensor of B elements; T = T_a T_b (T_b may be None).  -> Moved: the resized disparity, the three outputs (None where not asked
    for), the Splat of all planes ([moved candidates | costs | moved local maps]) with its companion, and every source's landing (dropped
    ones included) with its companions"""
    B = prev_disp.shape[0]
    dt = prev_disp.dtype
    with torch.no_grad():
        pd, apd = resize_disparity(prev_disp, h, w)
        K4 = _pad4(K).clone()
        K4[:, :2] = K4[:, :2] / factor
        iK = torch.inverse(K4[:, :3, :3])
        T, AT = (T_a, T_a.abs()) if T_b is None else (torch.matmul(T_a, T_b), torch.matmul(T_a.abs(), T_b.abs()))
        P, AP = torch.matmul(K4, T)[:, :3], torch.matmul(K4.abs(), AT)[:, :3]
        bf = (baseline.reshape(B).to(dt) * K4[:, 0, 0]).view(B, 1, 1, 1)
        r, Ar = _rays(iK, h, w)
        el = lambda i, j: P[:, i, j].reshape(-1, 1, 1, 1)
        slope = [el(i, 0) * r[:, 0] + el(i, 1) * r[:, 1] + el(i, 2) * r[:, 2] for i in range(3)]          # d cam / d depth, [B, 1, h, w] each

        def depth(d, ad):
            """-> z = bf / (d + 1e-5), the companion of its own roundings, and what the input's error beyond one rounding moves it by
            (kept apart: the sensitivity of what follows to the depth is taken exactly, not through absolute values -- a far plane's
            depth is ill-conditioned, its landing is not)"""
            z = bf / (d + 1e-5)
            return z, z.abs() * (1 + (d.abs() + 1e-5) / (d + 1e-5).abs()), z.abs() * (ad - d.abs()).clamp(min=0) / (d + 1e-5).abs()
        z0, az0, dz0 = depth(pd, apd)
        cam, acam = _move(P, AP, r, Ar, z0, az0)
        u = torch.arange(w, dtype=dt).view(1, 1, 1, w)
        v = torch.arange(h, dtype=dt).view(1, 1, h, 1)
        den = cam[:, 2] + 1e-7
        ox, oy = u + (cam[:, 0] / den - u), v + (cam[:, 1] / den - v)
        dx = (acam[:, 0] + ox.abs() * acam[:, 2]) / den.abs() + ox.abs() + ((slope[0] * den - cam[:, 0] * slope[2]) / (den * den)).abs() * dz0
        dy = (acam[:, 1] + oy.abs() * acam[:, 2]) / den.abs() + oy.abs() + ((slope[1] * den - cam[:, 1] * slope[2]) / (den * den)).abs() * dz0
        bad = ~(torch.isfinite(dx) & torch.isfinite(dy))
        dx, dy = torch.where(bad, torch.zeros_like(dx), dx), torch.where(bad, torch.zeros_like(dy), dy)
        foot = footprint(ox[:, 0], oy[:, 0], h, w)
        mean = pd.mean()
        metric = (pd - mean).clamp(-50, 50)

        def moved(d, ad):                # disparity -> depth -> rigid motion -> depth -> disparity, with its companion
            z, az, dz = depth(d, ad)
            mz, amz = _move(P, AP, r, Ar, z, az)
            val = bf / (mz[:, 2] + 1e-5)
            return val, (bf.abs() + val.abs() * (amz[:, 2] + 1e-5)) / (mz[:, 2] + 1e-5).abs() + (val * slope[2] / (mz[:, 2] + 1e-5)).abs() * dz
        k = 0 if mem_disp is None else mem_disp.shape[1]
        vals, comps = [], []
        if k:
            md, amd = moved(mem_disp, mem_disp.abs())
            vals += [md, mem_cost]
            comps += [amd, mem_cost.abs()]
        if n_local_out:
            lm, alm = (pd, apd) if local_map is None else (torch.cat([pd, local_map], 1)[:, :n_local_out], torch.cat([apd, local_map.abs()], 1)[:, :n_local_out])
            ml, aml = moved(lm, alm)
            vals.append(ml)
            comps.append(aml)
        s = splat_companions(foot, torch.cat(vals, 1), metric.exp(), 1 + apd + mean.abs(), torch.cat(comps, 1), dx[:, 0], dy[:, 0])
        return Moved(pd, s.out[:, :k] if k else None, s.out[:, k:2 * k] if k else None, s.out[:, 2 * k:] if n_local_out else None, s, foot, k, n_local_out,
                     ox[:, 0], oy[:, 0], dx[:, 0], dy[:, 0])
