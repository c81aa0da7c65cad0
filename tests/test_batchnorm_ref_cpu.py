"""tests/bn_ref.py (the float64 restatement that tests/test_batchnorm_gpu.py holds the BatchNorm kernels to) pinned to the framework,
the fp32 yardstick figures of tests/bn_cases.py pinned to what they measure, and the bounds shown to be tight: a reference with one
planted error lies outside them on the very inputs the GPU test uses.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

import bn_cases as K
import bn_ref
import synth

ACTS = (bn_ref.ACT_NONE, bn_ref.ACT_SILU, bn_ref.ACT_RELU)


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(K.TINY))


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("shape,affine", [((2, 3, 77), True), ((3, 5, 8), True), ((1, 2, 1024), False)])
def test_reference_agrees_with_the_framework_in_float64(shape, affine, act, train):
    """F.batch_norm (float64) + F.silu / F.relu and its autograd gradients against bn_ref, to 1e-12 relative; running statistics too"""
    B, C, N = shape
    x32 = torch.from_numpy(synth.normal(11, "x", shape)) * torch.tensor([1.0, 3.0, 0.5, 10.0, 2.0][:C]).view(1, C, 1) + 0.7
    dy32 = torch.from_numpy(synth.normal(11, "dy", shape))
    g32 = torch.from_numpy(synth.uniform(11, "g", (C,), 0.5, 1.5)) if affine else None
    b32 = torch.from_numpy(synth.normal(11, "b", (C,), 0.2)) if affine else None
    rm32, rv32 = torch.from_numpy(synth.normal(11, "rm", (C,), 0.2)) + 0.7, torch.from_numpy(synth.uniform(11, "rv", (C,), 0.5, 1.5))
    eps, momentum = 1e-3, 0.3
    x = x32.double().requires_grad_(True)
    g = g32.double().requires_grad_(True) if affine else None
    b = b32.double().requires_grad_(True) if affine else None
    rm, rv = rm32.double().clone(), rv32.double().clone()
    z = F.batch_norm(x, rm, rv, g, b, train, momentum, eps)
    y = F.silu(z) if act == bn_ref.ACT_SILU else F.relu(z) if act == bn_ref.ACT_RELU else z
    y.backward(dy32.double())
    if train:
        out, mean, var, running = bn_ref.bn_act_fwd(x32, g32, b32, eps, act, momentum=momentum, running=(rm32, rv32))
        assert _rel(running[0], rm) < 1e-12 and _rel(running[1], rv) < 1e-12
    else:
        out, mean, var, running = bn_ref.bn_act_fwd(x32, g32, b32, eps, act, mean=rm32, var=rv32)
        assert running is None and torch.equal(rm, rm32.double()) and torch.equal(rv, rv32.double())
    dx, s1, s2 = bn_ref.bn_act_bwd(x32, dy32, mean, var, g32, b32, eps, act, train, B * N)
    assert out.dtype == torch.float64 and _rel(out, y.detach()) < 1e-12
    assert _rel(dx, x.grad) < 1e-12
    if affine:
        assert _rel(s1, b.grad) < 1e-12 and _rel(s2, g.grad) < 1e-12


def test_running_variance_of_a_single_element_is_the_biased_one():
    x = torch.tensor([[[3.0]], ]).expand(1, 2, 1)
    _, mean, var, running = bn_ref.bn_act_fwd(x, None, None, 1e-5, 0, momentum=0.5, running=(torch.zeros(2), torch.ones(2)))
    assert torch.equal(var, torch.zeros(2, dtype=torch.float64)) and torch.equal(running[1], torch.full((2,), 0.5, dtype=torch.float64))
    assert torch.equal(running[0], torch.full((2,), 1.5, dtype=torch.float64))


def test_merge_of_parts_is_the_statistics_of_the_whole():
    x = K.channel_data(5, "x", ("n01", "k1000", "tiny", "wide"), 6, 50)
    parts = (x[:1], x[1:4], x[4:])
    recs = [bn_ref.batch_stats(p) + (float(p.shape[0] * 50),) for p in parts]
    mean, var, running, inv = bn_ref.sync_merge(recs, 0.1, (torch.zeros(4), torch.ones(4)))
    wm, wv = bn_ref.batch_stats(x)
    assert _rel(mean, wm) < 1e-12 and _rel(var, wv) < 1e-9 and inv == 1.0 / 300
    want = bn_ref.running_update(wm, wv, 300, 0.1, (torch.zeros(4), torch.ones(4)))
    assert _rel(running[0], want[0]) < 1e-12 and _rel(running[1], want[1]) < 1e-9


# ---- the yardstick figures written in bn_cases.YARD ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.CASES, ids=[c.name for c in K.CASES])
def test_written_yardstick_is_what_the_fp32_two_pass_form_measures(case):
    """every hard kind of channel of the case has its figure, the figure is the measurement (2 %: it is written with three digits), and
    so is the bound that follows from it"""
    m = K.measure(case)
    w = K.YARD.get(case.name, {})
    assert set(m) == set(w)
    for kind in m:
        for i, base in enumerate((K.BASE["out"], K.BASE["grad"], K.BASE["grad"])):
            bm, bw = max(base, 4 * m[kind][i]), max(base, 4 * w[kind][i])
            assert abs(bm - bw) <= 0.02 * bw, (kind, i, m[kind][i], w[kind][i])
            if 4 * w[kind][i] > base:
                assert abs(m[kind][i] - w[kind][i]) <= 0.02 * w[kind][i], (kind, i, m[kind][i], w[kind][i])
    b = K.bounds(case)
    hard = K.hard_channels(case)
    for key, base in (("out", K.BASE["out"]), ("dx", K.BASE["grad"]), ("s", K.BASE["grad"])):
        assert bool((b[key] >= base).all()) and bool((b[key][~hard] == base).all())


def test_every_kind_of_channel_and_every_layout_is_used():
    kinds = set(k for c in K.CASES for k in K.case_kinds(c))
    assert kinds == set(K.KINDS)
    for form in ("small", "two"):
        assert {(c.layout, c.act) for c in K.CASES if c.form == form} == {(L, a) for L in range(4) for a in ACTS}
    assert {c.momentum for c in K.CASES} == {0.0, 0.1, 1.0}
    assert any(not c.affine for c in K.CASES) and any(not c.running for c in K.CASES) and any(c.gamma == "g40" for c in K.CASES)
    # gamma = 40 reaches both saturation branches of the fast sigmoid (e^-z overflows below -88.7) and ReLU's z == 0
    for c in K.CASES:
        if c.gamma == "g40":
            d = K.make_inputs(c)
            ref = bn_ref.bn_act_fwd(d["x"], d["gamma"], d["beta"], d["eps"], bn_ref.ACT_NONE)[0]
            assert float(ref.min()) < -100 and float(ref.max()) > 100 and bool((ref == 0).any())


@pytest.mark.parametrize("case", K.EVAL_CASES, ids=[c.name for c in K.EVAL_CASES])
def test_eval_cases_are_well_conditioned(case):
    """the base bounds of the eval test stand: 4 x the fp32 yardstick of its inputs is below them"""
    d = K.eval_inputs(case)
    B, C, N = case.shape
    o, dx, _, _ = K.yardstick_terms(d["x"], d["dy"], d["mean"].double(), d["var"].double(), d["gamma"], d["beta"], d["eps"], case.act, False, B * N)
    ro = bn_ref.bn_act_fwd(d["x"], d["gamma"], d["beta"], d["eps"], case.act, mean=d["mean"], var=d["var"])[0]
    rdx = bn_ref.bn_act_bwd(d["x"], d["dy"], d["mean"], d["var"], d["gamma"], d["beta"], d["eps"], case.act, False, B * N)[0]
    assert 4 * float(K.err_planes(o, ro).max()) <= K.BASE["out"]
    assert 4 * float(K.err_planes(dx, rdx).max()) <= K.BASE["grad"]


# ---- sensitivity: one planted error at a time ------------------------------------------------------------------------------------
def _flawed(case, d, flaw):
    B, C, N = case.shape
    out, mean, var, running = bn_ref.bn_act_fwd(d["x"], d["gamma"], d["beta"], d["eps"], case.act, momentum=d["momentum"], running=d["running"], flaw=flaw)
    dx, s1, s2 = bn_ref.bn_act_bwd(d["x"], d["dy"], mean, var, d["gamma"], d["beta"], d["eps"], case.act, True, B * N, flaw=flaw)
    return {"out": out, "mean": mean, "var": var, "running": running, "dx": dx, "s1": s1, "s2": s2}


@pytest.mark.parametrize("case", K.CASES, ids=[c.name for c in K.CASES])
def test_bounds_notice_each_planted_error(case):
    """On the case's own input, at the case's own bounds: the reference with one planted error differs from the true one by more than
    the bound in at least one channel of the quantity the error touches -- a kernel with that error would fail the GPU test.
    Not asked where the error cannot show by construction: the running variance with momentum 0, without running statistics or
    with B * N == 1 (biased == unbiased); the s2 term of dx and the place of eps with B * N == 1 (xhat == 0, so out == beta and
    dx == 0 whatever invstd is); SiLU's derivative without SiLU."""
    B, C, N = case.shape
    d = K.make_inputs(case)
    ref = K.reference(case, d)
    bnd = K.bounds(case)
    sm, sv, srm, srv = K.stat_scales(ref["mean"], ref["var"], B * N, d["running"])

    def seen(flaw):
        f = _flawed(case, d, flaw)
        e = K.errors(f, ref)
        hit = {"out": bool((e["out"] > bnd["out"]).any()), "dx": bool((e["dx"] > bnd["dx"]).any()),
               "s": bool((e["s1"] > bnd["s"]).any() or (e["s2"] > bnd["s"]).any())}
        if d["running"] is not None:
            hit["running_var"] = bool((K.err_vec(f["running"][1], ref["running"][1], srv) > K.BASE["stat"]).any())
        return hit

    if d["running"] is not None and case.momentum > 0 and B * N > 1:
        assert seen("biased_running_var")["running_var"]
    if B * N > 1:
        assert seen("dx_without_s2_term")["dx"]
    assert seen("s1_s2_swapped")["s"]
    if B * N > 1:
        hit = seen("eps_outside_sqrt")
        assert hit["out"] or hit["dx"] or hit["s"]
    if case.act == bn_ref.ACT_SILU:
        hit = seen("silu_grad_without_z_term")
        assert hit["dx"] and hit["s"]


@pytest.mark.parametrize("world", [2, 3, 5])
@pytest.mark.parametrize("C", [1, 64, 65, 130])
def test_statistics_bound_notices_a_merge_without_the_mean_term(world, C):
    recs = K.merge_records(world, C)
    mean, var, _, _ = bn_ref.sync_merge(recs)
    _, bad, _, _ = bn_ref.sync_merge(recs, flaw="merge_without_d2")
    assert float(K.err_vec(bad, var, var).min()) > K.BASE["stat"]
