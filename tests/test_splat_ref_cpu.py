"""CPU: pins tests/splat_ref.py and tests/splat_cases.py, the reference and the cases of tests/test_splat_forms_gpu.py.

The float64 restatement equals oracle.splat, oracle.geometry and oracle.temporal in float64 to 1e-12 (of its own companion, which is
>= |value|); in fp32 it stays within the existing tolerances of tests/golden/project_to_3d*.npz and temporal_update_*.npz; the analytic
answers of tests/test_oracle_splat.py hold for it; dropped pixels -- absurd flows included -- deposit nothing and have zero gradients;
the stage-by-stage gradients are autograd's; companions are >= |value|; every case's yardstick is finite; the excused shares stay under the cap with the fp32 restatement standing in for the kernel; the edge-hugging
flows reach all nine combinations of inside flags and flow_mask takes both values on at least 10 % of some case's pixels.  The last
test is the K2 part of the ABI's argument checks, which return before any launch and so need no GPU.
"""
import numpy as np
import pytest
import torch

import oracle
import splat_cases as K
import splat_ref as R
from helpers import check_temporal_update, load, t
from oracle import geometry as ogeometry
from oracle import temporal as otemporal

F32, F64 = torch.float32, torch.float64
_ids = lambda c: c.name
SMALL = [c for c in K.SPLAT if c.H * c.W <= 64 * 64]
FINITE = [c for c in SMALL if c.field != "absurd"]


def _within(a, b, comp, tol=1e-12):
    """|a - b| <= tol * companion everywhere (the companion is >= |value|; where it is 0 both are exactly 0)"""
    return bool(((a - b).abs() <= tol * comp).all())


def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=F64)


# ---- the restatement is the oracle -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", FINITE, ids=_ids)
def test_float64_restatement_is_oracle_splat(case):
    inp, flow, metric, _ = [x.double() for x in K.splat_inputs(case)]
    for mode in R.MODES:
        m = None if mode in ("summation", "average") else (metric.abs() + 0.1 if mode == "linear" else metric)
        s, _ = R.splat_reference(inp, flow, m, mode)
        assert _within(s.out, oracle.softsplat(inp, flow, m, mode), s.comp), mode
        assert torch.equal(R.softsplat(inp, flow, m, mode), s.out), mode
        assert bool((s.comp >= s.out.abs()).all()), mode


@pytest.mark.parametrize("case", K.PROJECT, ids=_ids)
def test_float64_restatement_is_oracle_project_to_3d(case):
    ins = [x.double() for x in K.project_inputs(case)]
    p = R.project(*ins, eps=case.eps)
    o = ogeometry.project_to_3d(*ins, eps=case.eps)
    assert _within(p.tri, o["triangular_depth"], p.a_tri) and _within(p.flow, o["optical_flow"], p.a_flow)
    assert torch.equal(p.mask, o["flow_mask"])
    assert bool((p.a_tri >= p.tri.abs()).all()) and bool((p.a_flow >= p.flow.abs()).all())
    assert bool(torch.isfinite(p.flow).all()) and bool(torch.isfinite(p.tri).all())


@pytest.mark.parametrize("case", K.REPROJECT, ids=_ids)
def test_float64_restatement_is_oracle_temporal(case):
    c = case
    ins = {k: (v.double() if torch.is_tensor(v) else v) for k, v in K.reproject_inputs(c).items()}
    m64, _, _ = K.reproject_reference(c)
    T = ins["T_a"] if ins["T_b"] is None else torch.bmm(ins["T_a"], ins["T_b"])
    base = ins["baseline"].view(-1, 1, 1, 1)
    comp = K.split_planes(m64.splat.comp, c.k, c.n_out)
    if c.k:
        o = otemporal.update_past_cost(ins["prev_disp"], {"disp_sample": ins["mem_disp"], "cost_volume": ins["mem_cost"]}, ins["K"], T, base, c.Wf)
        assert _within(m64.disp, o["disp_sample"], comp[0]) and _within(m64.cost, o["cost_volume"], comp[1])
    if c.n_out and (ins["local_map"] is not None or (c.Hf // 8, c.Wf // 8) == (c.h, c.w)):
        o = otemporal.update_local_map(ins["prev_disp"], ins["local_map"], ins["K"], T, base, c.Hf, c.Wf, c.n_out)
        assert _within(m64.local, o, comp[2])
    assert bool((m64.splat.comp >= m64.splat.out.abs()).all()) and bool(torch.isfinite(m64.splat.out).all())
    pd = torch.nn.functional.interpolate(ins["prev_disp"] * c.w / c.Wf, size=(c.h, c.w), mode="bilinear", align_corners=True)
    assert _within(m64.pd, pd, R.resize_disparity(ins["prev_disp"], c.h, c.w)[1])


# ---- in fp32 it stays within the tolerances of the recorded vectors --------------------------------------------------------------
@pytest.mark.parametrize("name", ["project_to_3d", "project_to_3d_k3"])
def test_fp32_restatement_against_recorded_project_to_3d(name):
    g = load(name)
    Km = t(g["K"])
    inv_K = torch.inverse(Km) if Km.shape[-1] == 4 else torch.inverse(Km[:, :3, :3])
    p = R.project(t(g["depth"]), Km, inv_K, t(g["T"]))
    np.testing.assert_allclose(p.tri.numpy(), g["triangular_depth"], rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(p.flow.numpy(), g["optical_flow"], rtol=1e-5, atol=1e-4)
    if "flow_mask" in g:
        assert (p.mask.numpy() == g["flow_mask"]).all()


@pytest.mark.parametrize("case", range(5))
def test_fp32_restatement_against_recorded_update_map(case):
    g = load("temporal_update_%d" % case)
    use_cost, size = bool(int(g["use_past_cost"])), int(g["local_map_size"])
    local = t(g["local_map_in"]) if int(g["has_local_in"]) else None
    H, W = (int(v) for v in g["full_hw"])
    h, w = g["mem_disp_sample"].shape[-2:]
    T_a, T_b = (torch.bmm(t(g["T_now"]), t(g["inv_T_past"])), None) if int(g["composed"]) else (t(g["T_now"]), t(g["inv_T_past"]))
    n_out = 0 if size == 0 else (1 if local is None else size)
    m = R.reproject(t(g["prev_disp"]), t(g["mem_disp_sample"]) if use_cost else None, t(g["mem_cost_volume"]) if use_cost else None, local, n_out,
                    t(g["K"]), T_a, T_b, t(g["baseline"]).reshape(-1), float(W) / w, h, w)
    info = {"cost_memory": {"disp_sample": m.disp, "cost_volume": m.cost} if use_cost else None, "use_past_cost": use_cost}
    if n_out:
        info.update(local_map=m.local, local_map_size=size)
    check_temporal_update(g, info, 2e-5, 1e-4)


# ---- the analytic answers of tests/test_oracle_splat.py --------------------------------------------------------------------------
def test_analytic_answers():
    x = _rand(2, 3, 5, 7)
    zero = torch.zeros(2, 2, 5, 7, dtype=F64)
    assert torch.equal(R.splat_sum(x, zero), x)                                       # zero flow is the identity
    x = _rand(1, 2, 6, 8, seed=1)
    flow = torch.zeros(1, 2, 6, 8, dtype=F64)
    flow[:, 0], flow[:, 1] = 3.0, -2.0
    want = torch.zeros_like(x)
    want[:, :, 0:4, 3:8] = x[:, :, 2:6, 0:5]
    assert torch.equal(R.splat_sum(x, flow), want)                                    # an integer flow shifts, the rest is dropped
    x = _rand(1, 1, 9, 9, seed=2).abs()
    x[:, :, -1, :], x[:, :, :, -1] = 0, 0
    flow = torch.zeros(1, 2, 9, 9, dtype=F64)
    flow[:, 0], flow[:, 1] = 0.3, 0.6
    assert abs(float(R.splat_sum(x, flow).sum() - x.sum())) < 1e-12                   # mass is conserved inside the frame
    x = torch.zeros(1, 1, 4, 4, dtype=F64)
    x[0, 0, 1, 1] = 1.0
    flow = torch.zeros(1, 2, 4, 4, dtype=F64)
    flow[0, 0, 1, 1], flow[0, 1, 1, 1] = 0.25, 0.5
    out = R.splat_sum(x, flow)[0, 0]
    np.testing.assert_allclose([out[1, 1], out[1, 2], out[2, 1], out[2, 2]], [0.375, 0.125, 0.375, 0.125])
    x, flow = _rand(2, 3, 6, 6, seed=3), _rand(2, 2, 6, 6, seed=4) * 1.5
    m = torch.full((2, 1, 6, 6), 0.7, dtype=F64)
    np.testing.assert_allclose(R.softsplat(x, flow, m, "softmax").numpy(), R.softsplat(x, flow, None, "average").numpy(), rtol=1e-10, atol=1e-12)
    with pytest.raises(ValueError):
        R.softsplat(x, flow, m, "bogus")
    x = _rand(1, 2, 4, 5, seed=8).requires_grad_()
    flow = (_rand(1, 2, 4, 5, seed=9) * 0.8 + 0.13).requires_grad_()
    assert torch.autograd.gradcheck(R.splat_sum, (x, flow), eps=1e-6, atol=1e-6)


# ---- gradients: dropped pixels, and the stage-by-stage backward is autograd's ----------------------------------------------------
def _autograd(inp, flow, metric, mode, gout, pos_dtype):
    leaves = [x.clone().requires_grad_() for x in (inp, flow)] + ([metric.clone().requires_grad_()] if metric is not None else [])
    out = R.softsplat(leaves[0], leaves[1], leaves[2] if metric is not None else None, mode, pos_dtype)
    return dict(zip(("input", "flow", "metric"), torch.autograd.grad(out, leaves, gout)))


@pytest.mark.parametrize("case", [c for c in SMALL if c.field in ("noise", "edge", "collide", "absurd", "shift_neg")], ids=_ids)
def test_stage_by_stage_gradients_are_autograd_and_dropped_pixels_have_none(case):
    inp, flow, metric, gout = [x.double() for x in K.splat_inputs(case)]
    with torch.no_grad():
        ox, oy, _ = R.positions(flow, F32)
        dropped = ~R.footprint(ox, oy, case.H, case.W).alive.unsqueeze(1)
    if case.field == "absurd":
        assert int(dropped.sum()) >= min(len(K.ABSURD), case.H * case.W) - 1 and not bool(torch.isfinite(flow).all())
    for mode in R.MODES:
        m = None if mode in ("summation", "average") else (metric.abs() + 0.1 if mode == "linear" else metric)
        auto = _autograd(inp, flow, m, mode, gout, F32)
        mine = R.softsplat_grads(inp, flow, m, mode, gout, F32)
        for q, g in auto.items():
            if q == "metric" and mode not in ("linear", "softmax"):
                continue
            val, comp = mine[q]
            assert bool(torch.isfinite(g).all()), (mode, q)
            assert _within(val, g, comp, 1e-11), (mode, q)
            assert bool((comp >= val.abs() * (1 - 1e-12)).all()), (mode, q)
            assert float((g * dropped).abs().max()) == 0.0, (mode, q, "a dropped pixel has a gradient")


# ---- yardsticks, excused shares, coverage ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.SPLAT, ids=_ids)
def test_splat_yardsticks_are_finite_and_excused_shares_under_the_cap(case):
    refs = K.splat_reference(case)
    for mode, r in refs.items():
        assert bool(torch.isfinite(r["fp32"]).all())
        for kind in ("mixed", "exact"):
            for extra in (None,) + ((K.FIX_HALF * r[kind].splat.count,) if mode == "summation" else ()):
                _, yard, bnd, share = K.judge(r["fp32"], r["fp32"], r[kind], extra)
                assert np.isfinite(yard) and yard <= bnd, (mode, kind, yard)
                assert share <= K.MAX_EXCUSED and (kind == "exact" or share == 0.0), (mode, kind, share)
    g64, g32 = K.grad_reference(case)
    assert np.isfinite(K.units(g32[0], g64[0], g64[1])) and np.isfinite(K.units(g32[1], g64[2], g64[3]))
    if case.field == "zero":
        assert torch.equal(refs["summation"]["mixed"].splat.out.float(), K.splat_inputs(case)[0])


@pytest.mark.parametrize("case", K.PROJECT, ids=_ids)
def test_project_yardsticks_and_mask_shares(case):
    p64, p32 = K.project_reference(case)
    j = K.judge_project(p32.tri, p32.flow, p32.mask, case)
    assert all(np.isfinite(j[q][1]) and j[q][0] <= j[q][2] for q in ("tri", "flow"))
    assert j["mask"][0] == 0 and j["mask"][1] <= K.MAX_EXCUSED


def test_flow_mask_takes_both_values():
    shares = [float(K.project_reference(c)[0].mask.double().mean()) for c in K.PROJECT]
    assert any(0.1 <= s <= 0.9 for s in shares), shares


@pytest.mark.parametrize("case", K.REPROJECT, ids=_ids)
def test_reproject_yardsticks_and_excused_shares(case):
    m64, ref, m32 = K.reproject_reference(case)
    _, yard, bnd, share = K.judge(m32.splat.out, m32.splat.out, ref)
    assert np.isfinite(yard) and yard <= bnd and share <= K.MAX_EXCUSED, (yard, share)
    assert bool(torch.isfinite(m32.splat.out).all())
    ins = K.reproject_inputs(case)
    assert bool((ins["prev_disp"] == 0).any()) and float(ins["prev_disp"].max()) <= 60.0


def test_case_tables_reach_what_they_are_for():
    big = [c for c in K.SPLAT if c.B * c.H * c.W > K.GRID_CAP_PIXELS]
    assert big and all((c.B - 1) * c.H * c.W < K.GRID_CAP_PIXELS for c in big)                # the wrapped pixels lie in the last item
    assert any(c.C * c.H * c.W > K.GRID_CAP_PIXELS for c in K.PROJECT)
    assert any(c.B * c.h * c.w > K.MAX_PARTS_PIXELS for c in K.REPROJECT)
    assert any(c.h == 1 and c.w == 1 for c in K.REPROJECT) and any(c.gap and c.k_dim == 3 and c.per_item_baseline for c in K.REPROJECT)
    assert {(c.k_dim, c.inv_k_dim) for c in K.PROJECT} == {(3, 3), (3, 4), (4, 3), (4, 4)} and {c.eps for c in K.PROJECT} == {1e-7, 1e-3}
    case = next(c for c in K.SPLAT if c.field == "edge" and (c.H, c.W) == (17, 31))
    ox, oy, _ = R.positions(K.splat_inputs(case)[1])
    x0, y0 = torch.floor(ox), torch.floor(oy)
    state = lambda a0, n: ((a0 >= 0) & (a0 < n)).long() * 2 + ((a0 + 1 >= 0) & (a0 + 1 < n)).long()      # 1: far tap only, 2: near tap only, 3: both
    seen = {(int(a), int(b)) for a, b in zip(state(x0, case.W).flatten(), state(y0, case.H).flatten())}
    assert {(a, b) for a in (1, 2, 3) for b in (1, 2, 3)} <= seen and any(0 in s for s in seen)
    case = next(c for c in K.SPLAT if c.field == "collide" and (c.H, c.W) == (17, 31))
    count = K.splat_reference(case)["summation"]["mixed"].splat.count
    assert int((count > 0).sum()) == 9 * case.B and float(count.max()) > 50


# ---- the ABI's argument checks: they return before any launch --------------------------------------------------------------------
def test_k2_entries_refuse_bad_arguments_without_gpu():
    from temporalstereo_amd import _lib
    L = _lib.lib()
    OK, NULL, SHAPE, UNSUP = K.TS_OK, K.TS_ERR_NULL, K.TS_ERR_SHAPE, K.TS_ERR_UNSUPPORTED
    assert L.ts_softsplat_softmax_workspace_bytes(0, 1, 1, 1) == 0 and L.ts_softsplat_softmax_workspace_bytes(1, 1, 1, -1) == 0
    up = lambda n: (n + 255) // 256 * 256
    assert L.ts_softsplat_softmax_workspace_bytes(2, 3, 5, 7) == up(2 * (3 + 1) * 5 * 7 * 4)
    assert L.ts_reproject_memory_workspace_bytes(0, 1, 1, 1, 1) == 0 and L.ts_reproject_memory_workspace_bytes(1, 1, 1, -1, 1) == 0
    assert L.ts_reproject_memory_workspace_bytes(1, 1, 1, 1, 1) == up((1 * (2 + 2 * 1 + 1) + 1024) * 4)
    assert L.ts_softsplat_sum_fwd(None, None, None, 1, 1, 0, 1, None) == SHAPE
    assert L.ts_softsplat_sum_fwd(None, None, None, 1, 1, 1, 1, None) == NULL
    assert L.ts_softsplat_sum_fwd_deterministic(None, None, None, None, 1, -1, 1, 1, None) == SHAPE
    assert L.ts_softsplat_softmax_fwd(None, None, None, None, None, 1, 1, 1, 1, None) == NULL
    assert L.ts_softsplat_sum_bwd_input(None, None, None, 1, 1, 1, 1, None) == NULL
    assert L.ts_softsplat_sum_bwd_flow(None, None, None, None, 0, 1, 1, 1, None) == SHAPE
    assert L.ts_project_to_3d_fwd(None, None, None, None, None, None, None, 1, 1, 1, 1, 5, 3, 1e-7, None) == SHAPE
    assert L.ts_project_to_3d_fwd(None, None, None, None, None, None, None, 1, 1, 1, 1, 3, 2, 1e-7, None) == SHAPE
    assert L.ts_project_to_3d_fwd(None, None, None, None, None, None, None, 65536, 1, 1, 1, 3, 3, 1e-7, None) == UNSUP
    assert L.ts_project_to_3d_fwd(None, None, None, None, None, None, None, 1, 1, 1, 1, 3, 3, 1e-7, None) == NULL
    rp = lambda k=1, n_in=0, n_out=1, k_dim=4, factor=8.0, B=1: L.ts_reproject_memory_fwd(None, 0, 8, 8, None, None, k, None, n_in, n_out, None, k_dim, None, None,
                                                                                            None, 0.5, factor, None, None, None, None, B, 1, 1, None)
    assert rp() == NULL and rp(k=0, n_out=0) == SHAPE and rp(n_in=1, n_out=3) == SHAPE and rp(k_dim=5) == SHAPE
    assert rp(factor=0.0) == SHAPE and rp(factor=-1.0) == SHAPE and rp(B=65536) == UNSUP and rp(B=0) == SHAPE
    assert OK == 0
