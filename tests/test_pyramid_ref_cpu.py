"""tests/pyramid_ref.py (the float64 restatement that tests/test_pyramid_ops_gpu.py holds the pyramid's element kernels to) pinned to
the framework's own float64 ops on every shape the framework accepts, three closed forms, and the fp32 yardstick figures of
tests/pyramid_cases.py pinned to what they measure.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

import pyramid_cases as K
import pyramid_ref as R
import synth


def _d(seed, tag, shape, scale=1.0):
    return torch.from_numpy(synth.normal(seed, tag, shape, scale)).double()


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(K.TINY))


# ---- the reference against the framework -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("content", ["n01", "quant", "neg", "const"])
@pytest.mark.parametrize("shape", [s for s in K.POOL_SHAPES if min(s[2:]) >= 5] + [(2, 2, 5, 5, 5), (1, 2, 6, 7, 9)])
def test_pool5_and_its_gradient_are_the_frameworks(shape, content):
    """F.avg_pool3d / F.max_pool3d (5, 1, 2) in float64 and their autograd: the max bit for bit, ties and all"""
    x = (K.pool_input(shape, content) if shape in K.POOL_SHAPES else torch.round(2 * _d(3, "x", shape)) / 2).double()
    ga, gm = _d(3, "ga", shape), _d(3, "gm", shape)
    xr = x.clone().requires_grad_(True)
    a, m = F.avg_pool3d(xr, 5, 1, 2), F.max_pool3d(xr, 5, 1, 2)
    (a * ga).sum().backward(retain_graph=True)
    gxa = xr.grad.clone()
    xr.grad = None
    (m * gm).sum().backward()
    avg, mx = R.pool5(x)
    assert torch.equal(mx, m.detach()) and _rel(avg, a.detach()) < 1e-13
    assert _rel(R.pool5_bwd(x, ga, torch.zeros_like(gm)), gxa) < 1e-13
    assert _rel(R.pool5_bwd(x, torch.zeros_like(ga), gm), xr.grad) < 1e-13
    assert _rel(R.pool5_bwd(x, ga, gm), gxa + xr.grad) < 1e-13


@pytest.mark.parametrize("src,dst", [(s, t) for s, t in K.R3_SHAPES] + [((2, 3, 4), (5, 4, 9))])
@pytest.mark.parametrize("act", [0, 1])
def test_resize3d_add_act_and_its_gradients_are_the_frameworks(src, dst, act):
    a, add, g = _d(4, "a", (2, 3) + src), _d(4, "b", (2, 3) + dst), _d(4, "g", (2, 3) + dst)
    ar, br = a.clone().requires_grad_(True), add.clone().requires_grad_(True)
    v = F.interpolate(ar, size=dst, mode="trilinear", align_corners=True) + br
    y = F.silu(v) if act else v
    y.backward(g)
    assert _rel(R.resize3d_add_act(a, add, dst, act), y.detach()) < 1e-13
    ga, gb = R.resize3d_add_act_bwd(a, add, g, dst, act)
    assert _rel(ga, ar.grad) < 1e-12 and _rel(gb, br.grad) < 1e-13
    no_add = R.resize3d_add_act(a, None, dst, 0)
    assert _rel(no_add, F.interpolate(a, size=dst, mode="trilinear", align_corners=True)) < 1e-13


@pytest.mark.parametrize("src,dst", K.BIL_SHAPES)
def test_resize_bilinear_is_the_frameworks(src, dst):
    x = K.bil_input(src).double()
    assert _rel(R.resize_bilinear(x, dst, 2.5), F.interpolate(x * 2.5, size=dst, mode="bilinear", align_corners=True)) < 1e-13


@pytest.mark.parametrize("case", [c for c in K.MERGE_FWD if c.layout == "dense" and c.C == 3 and c.hw == (3, 5)], ids=lambda c: c.name)
def test_merge_is_sort_and_gather(case):
    """torch.sort(stable) + gather on the concatenation, the memory half written out by hand; merge_bwd against autograd"""
    d = K.merge_input(case)
    out_s, out_v, order = K.merge_reference(d)
    B, C, D0, H, W = d["vol"].shape
    s = K.merge_cat_sample(d).double()
    vol = d["vol"].double()
    if d["K"]:
        mc = torch.zeros(B, d["K"], H, W, dtype=torch.float64) if d["mem_cost"] is None else d["mem_cost"].double()
        z = torch.stack([d["w"][c].double() * mc * d["scale"][c].double() + d["shift"][c].double() for c in range(C)], 1)
        vol = torch.cat([vol, F.silu(z)], 2)
    vol.requires_grad_(True)
    s.requires_grad_(True)
    ss, idx = torch.sort(s, dim=1, stable=True)
    gathered = torch.gather(vol, 2, idx.unsqueeze(1).expand(-1, C, -1, -1, -1))
    assert torch.equal(ss.detach(), out_s) and torch.equal(idx, order) and _rel(out_v, gathered.detach()) < 1e-14
    assert bool((out_s[:, 1:] >= out_s[:, :-1]).all())
    gv, gs = _d(5, "gv", tuple(gathered.shape)), _d(5, "gs", tuple(ss.shape))
    ((gathered * gv).sum() + (ss * gs).sum()).backward()
    rv, rs = R.merge_bwd(s.detach(), gv, gs)
    assert torch.equal(rv, vol.grad) and torch.equal(rs, s.grad)
    assert not bool(R.merge_bwd(s.detach(), gv, None)[1].any())


def test_merge_inputs_hold_the_ties_they_promise():
    for case in K.MERGE_FWD:
        if case.layout != "dense" or case.DT == 1 or case.form == "i0":       # one candidate, or the candidates 0 .. D0-1 themselves
            continue
        s = K.merge_cat_sample(K.merge_input(case))
        srt = torch.sort(s, dim=1)[0]
        tied = ((srt[:, 1:] == srt[:, :-1]).any(1)).float().mean()
        assert float(tied) >= 0.3, case.name
        assert bool(((s == 0) & torch.signbit(s)).any()) and bool(((s == 0) & ~torch.signbit(s)).any()), case.name


def test_range_candidates_formula():
    d = torch.tensor([[[10.0, 3.0]]], dtype=torch.float64)
    low, high, cand = R.range_candidates(d, -2.0)              # low > high: |.| and min() put the candidates back in ascending order
    assert low.tolist() == [[[12.0, 5.0]]] and high.tolist() == [[[8.0, 1.0]]]
    assert cand[0, :, 0, 0].tolist() == [8.0, 9.5, 10.0, 10.5, 12.0]
    assert R.range_candidates(d, 0.0)[2][0, :, 0, 1].tolist() == [3.0] * 5


# ---- closed forms ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", K.POOL_SHAPES)
def test_constant_volume_sends_every_window_to_its_first_element(shape):
    """all values equal: the first maximum in (d, y, x) order is the window's first in-bounds element (max(d-2,0), max(y-2,0), max(x-2,0))"""
    B, C, D, H, W = shape
    gm = _d(6, "gm", shape)
    got = R.pool5_bwd(torch.full(shape, 1.5, dtype=torch.float64), torch.zeros(shape, dtype=torch.float64), gm)
    want = torch.zeros(B, C, D * H * W, dtype=torch.float64)
    d, y, x = torch.meshgrid(torch.arange(D), torch.arange(H), torch.arange(W), indexing="ij")
    flat = ((d - 2).clamp(min=0) * H + (y - 2).clamp(min=0)) * W + (x - 2).clamp(min=0)
    want.scatter_add_(2, flat.reshape(1, 1, -1).expand(B, C, -1), gm.reshape(B, C, -1))
    assert torch.equal(got, want.reshape(shape))


@pytest.mark.parametrize("shape", K.POOL_SHAPES)
def test_all_negative_volume_has_negative_border_maxima(shape):
    x = K.pool_input(shape, "neg").double()
    avg, mx = R.pool5(x)
    assert float(mx.max()) <= -0.5 and float(avg.max()) < 0 and bool(torch.isfinite(mx).all())


@pytest.mark.parametrize("src,dst", [(s, t) for s, t in K.R3_SHAPES if min(t) > 1])
def test_align_corners_output_corners_are_the_source_corners(src, dst):
    for dtype in (torch.float64, torch.float32):
        a = _d(7, "a", (1, 2) + src).to(dtype)
        out = R.resize_linear(a, dst)
        for cd, ch, cw in [(i, j, k) for i in (0, -1) for j in (0, -1) for k in (0, -1)]:
            assert torch.equal(out[:, :, cd, ch, cw], a[:, :, cd, ch, cw])


# ---- the yardstick figures written in pyramid_cases.YARD -------------------------------------------------------------------------
_BASES = {"pool_": "avg", "poolbwd_": "grad", "merge_": "out", "resize_": "resize", "resizebwd_": "grad", "bilinear_": "out", "range_": "out",
          "unet_": "tol", "convex_": "tol"}


def test_every_case_has_its_yardstick():
    assert set(K.YARD) == set(K.measured())


@pytest.mark.parametrize("key", sorted(K.measured()))
def test_written_yardstick_is_what_float32_measures(key):
    """the figure is the measurement (2 %: it is written with three digits) wherever it sets the bound, and the bound that follows from
    the written figure is the one that follows from the measurement everywhere"""
    fn, case = K.measured()[key]
    base = K.BASE[_BASES[key.split("_")[0] + "_"]]
    m, w = fn(case), K.YARD[key]
    assert set(m) == set(w)
    for q in m:
        bm, bw = max(base, 4 * m[q]), max(base, 4 * w[q])
        assert abs(bm - bw) <= 0.02 * bw, (q, m[q], w[q])
        if 4 * w[q] > base:
            assert abs(m[q] - w[q]) <= 0.02 * w[q], (q, m[q], w[q])
