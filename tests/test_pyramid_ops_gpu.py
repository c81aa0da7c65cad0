"""GPU: the element kernels of csrc/pyramid_ops.hip called on their own through the C ABI (the two softmax upsamplers through their
autograd functions), against the float64 restatement tests/pyramid_ref.py, at the edge shapes of tests/pyramid_cases.py: tensors carved
out of sentinel-filled buffers with guard bands (tests/sentinel.py), so that every case also asserts that nothing but its outputs
changed -- inputs, neighbouring channels of a strided buffer, guard bands.

Per case: the status code; bit-for-bit equality of everything that is a move or a comparison (the pooled maximum, the sorted samples,
the gathered columns of computed candidates, all of the merge's backward, the pair form of the bilinear resize against two single
calls) -- ties and signed zeros included, nothing masked out; the bound of pyramid_cases (max(base, 4 x the fp32 yardstick), metric and
bases in its docstring) for everything else; every output finite; identical bits on a second call for the kernels without atomics.

`-s` prints case, quantity, error and bound; with TS_PYRAMID_PARITY_FILE set the same lines are appended to that file
(profiles/pyramid_ops_parity.txt).
"""
import os

import pytest
import torch

import pyramid_cases as K
import pyramid_ref as R
from sentinel import GUARD, Arena, dense

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_ids = lambda c: c.name


def _api():
    from temporalstereo_amd import _lib
    return _lib.lib(), _lib.current_stream_handle()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


def _within(case, quantity, err, bound):
    line = "%-46s %-12s %.3g (bound %.3g)" % (case, quantity, err, bound)
    print(line)
    if os.environ.get("TS_PYRAMID_PARITY_FILE"):
        with open(os.environ["TS_PYRAMID_PARITY_FILE"], "a") as f:
            f.write(line + "\n")
    assert err <= bound, line


def _same_bits(got, ref):
    """fp32 tensors equal bit for bit (0.0 and -0.0 differ); ref may be float64 holding fp32 values"""
    return torch.equal(got.detach().cpu().contiguous().view(torch.int32), ref.float().contiguous().view(torch.int32))


def _exact(case, quantity, got, ref):
    _within(case, quantity + " (bits)", 0.0 if _same_bits(got, ref) else float("inf"), 0.0)


def _run(arenas, call, want_rc=K.TS_OK, twice=True):
    """seal -> call -> nothing but the outputs changed; a second call on the restored buffers gives the same bits"""
    for a in arenas:
        a.seal()
    rc = call()
    torch.cuda.synchronize()
    assert rc == want_rc, "status %d, expected %d" % (rc, want_rc)
    assert all(a.intact() for a in arenas), "written outside the outputs"
    if twice and want_rc == K.TS_OK:
        first = [a.buf.clone() for a in arenas]
        for a in arenas:
            a.restore()
        assert call() == K.TS_OK
        torch.cuda.synchronize()
        assert all(torch.equal(a.buf.view(torch.int32), f.view(torch.int32)) for a, f in zip(arenas, first)), "a second call gives other bits"


def _finite(*ts):
    assert all(bool(torch.isfinite(t).all()) for t in ts), "non-finite output"


# ---- 5^3 avg + max pooling -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.POOL_FWD, ids=_ids)
def test_pool5_forward(case):
    L, stream = _api()
    B, C, D, H, W = case.shape
    n = D * H * W
    x = K.pool_input(case.shape, case.content)
    if case.layout == "dense":
        (ax, xv), (aa, av), (am, mv) = dense(case.shape, DEV, fill=x), dense(case.shape, DEV, out=True), dense(case.shape, DEV, out=True)
        arenas, bs = [ax, aa, am], C * n
    else:                                   # x = channel slice 0 of the engine's [B, 4C, D, H, W] buffer, avg -> slice 1, max -> slice 2
        A = Arena(B * 4 * C * n, DEV)
        st = (4 * C * n, n, H * W, W, 1)
        xv, av, mv = A.carve(case.shape, st, 0, fill=x), A.carve(case.shape, st, C * n, out=True), A.carve(case.shape, st, 2 * C * n, out=True)
        arenas, bs = [A], 4 * C * n
    _run(arenas, lambda: L.ts_pool3d5_avgmax_fwd(_ptr(xv), _ptr(av), _ptr(mv), B, C, D, H, W, bs, n, bs, n, bs, n, stream))
    ravg, rmax = R.pool5(x.double())
    _finite(av, mv)
    _exact(case.name, "max", mv, rmax)
    _within(case.name, "avg", K.err_planes(av, ravg), K.bound(case.key, "avg", K.BASE["avg"]))


@pytest.mark.parametrize("case", K.POOL_BWD, ids=_ids)
def test_pool5_backward(case):
    """grad_x = box(grad_avg) / 125 + grad_max at each window's FIRST maximum in (d, y, x) order: quantised and constant volumes tie in
    almost every window.  (LDS and global atomics: no second call.)"""
    L, stream = _api()
    B, C, D, H, W = case.shape
    x = K.pool_input(case.shape, case.content)
    for which in K.POOL_GRADS:
        ga, gm = K.pool_grads(case.shape, which)
        (ax, xv), (a1, gav), (a2, gmv), (ao, gxv) = dense(case.shape, DEV, fill=x), dense(case.shape, DEV, fill=ga), dense(case.shape, DEV, fill=gm), \
            dense(case.shape, DEV, out=True)
        _run([ax, a1, a2, ao], lambda: L.ts_pool3d5_avgmax_bwd(_ptr(xv), _ptr(gav), _ptr(gmv), _ptr(gxv), B, C, D, H, W, stream), twice=False)
        _finite(gxv)
        _within(case.name, "gx " + which, K.err_tensor(gxv, R.pool5_bwd(x.double(), ga.double(), gm.double())), K.bound(case.key, which, K.BASE["grad"]))


# ---- merge candidates ------------------------------------------------------------------------------------------------------------
def _merge_call(L, stream, d, C, hw, layout):
    """-> arenas, out_sample view, out_volume view, call"""
    B, D0, Kk, (H, W) = K.MERGE_B, d["D0"], d["K"], hw
    DT, n = D0 + Kk, hw[0] * hw[1]
    if layout == "dense":
        av, vol = dense((B, C, D0, H, W), DEV, fill=d["vol"])
        ao, ov = dense((B, C, DT, H, W), DEV, out=True)
        vbs, vcs, obs, ocs = C * D0 * n, D0 * n, C * DT * n, DT * n
    else:                                   # vol = channels C .. 2C-1 of a [B, 3C, D0, H, W] buffer, out = the first C channels of [B, 4C, DT, H, W]
        av, ao = Arena(B * 3 * C * D0 * n, DEV), Arena(B * 4 * C * DT * n, DEV)
        vbs, vcs, obs, ocs = 3 * C * D0 * n, D0 * n, 4 * C * DT * n, DT * n
        vol = av.carve((B, C, D0, H, W), (vbs, vcs, n, W, 1), C * D0 * n, fill=d["vol"])
        ov = ao.carve((B, C, DT, H, W), (obs, ocs, n, W, 1), 0, out=True)
    aos, osv = dense((B, DT, H, W), DEV, out=True)
    ins = {k: (None, None) if d[k] is None else dense(tuple(d[k].shape), DEV, fill=d[k]) for k in ("sample", "mem_sample", "mem_cost", "w", "scale", "shift")}
    p = {k: _ptr(v[1]) for k, v in ins.items()}
    call = lambda: L.ts_merge_candidates_fwd(_ptr(vol), p["sample"], p["mem_sample"], p["mem_cost"], p["w"], p["scale"], p["shift"], _ptr(osv), _ptr(ov),
                                             B, C, D0, Kk, H, W, vbs, vcs, obs, ocs, stream)
    return [av, ao, aos] + [v[0] for v in ins.values() if v[0] is not None], osv, ov, call


@pytest.mark.parametrize("case", K.MERGE_FWD, ids=_ids)
def test_merge_candidates_forward(case):
    L, stream = _api()
    d = K.merge_input(case)
    arenas, osv, ov, call = _merge_call(L, stream, d, case.C, case.hw, case.layout)
    _run(arenas, call)
    rs, rv, order = K.merge_reference(d)
    _finite(osv, ov)
    _exact(case.name, "sample", osv, rs)
    computed = (order < d["D0"]).unsqueeze(1).expand_as(rv)
    _exact(case.name, "computed", ov.cpu()[computed], rv[computed])
    _within(case.name, "volume", K.err_planes(ov, rv), K.bound(case.key, "vol", K.BASE["out"]))


@pytest.mark.parametrize("hw", K.MERGE_HW)
def test_merge_candidates_refuses_more_than_twenty(hw):
    L, stream = _api()
    B, C, D0, Kk = K.MERGE_B, 3, 12, 9
    d = {"D0": D0, "K": Kk, "vol": torch.zeros(B, C, D0, *hw), "sample": torch.zeros(B, D0, *hw), "mem_sample": torch.zeros(B, Kk, *hw),
         "mem_cost": torch.zeros(B, Kk, *hw), "w": torch.ones(C), "scale": torch.ones(C), "shift": torch.zeros(C)}
    arenas, osv, ov, call = _merge_call(L, stream, d, C, hw, "dense")
    _run(arenas, call, want_rc=K.TS_ERR_UNSUPPORTED)
    assert bool((osv == K.SENTINEL).all()) and bool((ov == K.SENTINEL).all())


@pytest.mark.parametrize("case", K.MERGE_BWD, ids=_ids)
def test_merge_candidates_backward(case):
    """the inverse permutation, bit for bit; a NULL grad_out_sample gives zeros, a NULL grad_sample leaves only the volume's gradient"""
    import synth
    L, stream = _api()
    B, C, DT, (H, W) = K.MERGE_B, case.C, case.DT, case.hw
    s = K.merge_cat_sample(K.merge_input(case))
    gov = torch.from_numpy(synth.normal(2350 + DT, "gv%d%d" % (C, H), (B, C, DT, H, W)))
    gos = torch.from_numpy(synth.normal(2350 + DT, "gs%d%d" % (C, H), (B, DT, H, W)))
    for form in ("full", "no_grad_out_sample", "no_grad_sample"):
        (a0, sv), (a1, govv), (a2, gosv) = dense(s.shape, DEV, fill=s), dense(gov.shape, DEV, fill=gov), dense(gos.shape, DEV, fill=gos)
        (a3, gv), (a4, gs) = dense(gov.shape, DEV, out=True), dense(gos.shape, DEV, out=(form != "no_grad_sample"))
        pgos, pgs = (None if form == "no_grad_out_sample" else _ptr(gosv)), (None if form == "no_grad_sample" else _ptr(gs))
        _run([a0, a1, a2, a3, a4], lambda: L.ts_merge_candidates_bwd(_ptr(sv), _ptr(govv), pgos, _ptr(gv), pgs, B, C, DT, H, W, stream))
        rv, rs = R.merge_bwd(s.double(), gov.double(), None if form == "no_grad_out_sample" else gos.double())
        _exact(case.name, "gvol " + form, gv, rv)
        if form != "no_grad_sample":
            _exact(case.name, "gsamp " + form, gs, rs)


# ---- trilinear resize + add + act ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.R3_FWD, ids=_ids)
def test_resize3d_add_act_forward(case):
    L, stream = _api()
    B, C = case.B, case.C
    a, add, _ = K.r3_input(case)
    na, n = _numel(case.src), _numel(case.dst)
    sa, so = (B, C) + case.src, (B, C) + case.dst
    if case.layout == "dense":
        (aa, av), (ao, ov) = dense(sa, DEV, fill=a), dense(so, DEV, out=True)
        ab, bv = dense(so, DEV, fill=add) if add is not None else (None, None)
        abs_, bbs, obs = C * na, C * n, C * n
    else:                                   # a = channels 1 .. C of [B, C+2, ...], add = the first C of [B, 2C, ...], out = the last C of [B, 2C+1, ...]
        aa, ab, ao = Arena(B * (C + 2) * na, DEV), (Arena(B * 2 * C * n, DEV) if add is not None else None), Arena(B * (2 * C + 1) * n, DEV)
        abs_, bbs, obs = (C + 2) * na, 2 * C * n, (2 * C + 1) * n
        tail = lambda s: (s[1] * s[2], s[2], 1)
        av = aa.carve(sa, (abs_, na) + tail(case.src), na, fill=a)
        bv = ab.carve(so, (bbs, n) + tail(case.dst), 0, fill=add) if add is not None else None
        ov = ao.carve(so, (obs, n) + tail(case.dst), (C + 1) * n, out=True)
    arenas = [x for x in (aa, ab, ao) if x is not None]
    _run(arenas, lambda: L.ts_resize3d_add_act_fwd(_ptr(av), _ptr(bv), _ptr(ov), B, C, *case.src, *case.dst, case.act, abs_, na, bbs, n, obs, n, stream))
    _finite(ov)
    ref = R.resize3d_add_act(a.double(), None if add is None else add.double(), case.dst, case.act)
    _within(case.name, "out", K.err_planes(ov, ref), K.bound(case.key, "out", K.BASE["resize"]))


@pytest.mark.parametrize("case", K.R3_BWD, ids=_ids)
def test_resize3d_add_act_backward(case):
    """(fp32 atomics into grad_a: no second call)"""
    L, stream = _api()
    B, C = case.B, case.C
    a, add, g = K.r3_input(case)
    sa, so = (B, C) + case.src, (B, C) + case.dst
    (aa, av), (ag, gv), (aga, gav) = dense(sa, DEV, fill=a), dense(so, DEV, fill=g), dense(sa, DEV, out=True)
    ab, bv = dense(so, DEV, fill=add) if add is not None else (None, None)
    agb, gbv = dense(so, DEV, out=True) if case.add == "add+g" else (None, None)
    arenas = [x for x in (aa, ag, aga, ab, agb) if x is not None]
    _run(arenas, lambda: L.ts_resize3d_add_act_bwd(_ptr(av), _ptr(bv), _ptr(gv), _ptr(gav), _ptr(gbv), B, C, *case.src, *case.dst, case.act, stream), twice=False)
    ra, rb = R.resize3d_add_act_bwd(a.double(), None if add is None else add.double(), g.double(), case.dst, case.act)
    _finite(gav)
    _within(case.name, "grad_a", K.err_tensor(gav, ra), K.bound(case.key, "grad_a", K.BASE["grad"]))
    if gbv is not None:
        _finite(gbv)
        _within(case.name, "grad_add", K.err_tensor(gbv, rb), K.bound(case.key, "grad_add", K.BASE["grad"]))


# ---- bilinear resize -------------------------------------------------------------------------------------------------------------
def _bilinear(L, stream, x, dst, vs, padded):
    B, C, (h, w), (Ho, Wo) = K.BIL_B, K.BIL_C, tuple(x.shape[2:]), dst
    ax, xv = dense(tuple(x.shape), DEV, fill=x)
    obs = (C + 2 if padded else C) * Ho * Wo
    ao = Arena(B * obs, DEV)
    ov = ao.carve((B, C, Ho, Wo), (obs, Ho * Wo, Wo, 1), 0, out=True)
    _run([ax, ao], lambda: L.ts_resize_bilinear_fwd(_ptr(xv), _ptr(ov), B, C, h, w, Ho, Wo, vs, obs, stream))
    return ov


@pytest.mark.parametrize("case", K.BIL, ids=_ids)
def test_resize_bilinear(case):
    L, stream = _api()
    x = K.bil_input(case.src)
    ov = _bilinear(L, stream, x, case.dst, case.vs, case.layout == "padded")
    _finite(ov)
    _within(case.name, "out", K.err_tensor(ov, R.resize_bilinear(x.double(), case.dst, case.vs)), K.bound(case.key, "out", K.BASE["out"]))


@pytest.mark.parametrize("case", K.BIL_PAIR, ids=_ids)
def test_resize_bilinear_pair_is_two_single_calls(case):
    L, stream = _api()
    B, C, (h, w), (Ho, Wo) = K.BIL_B, K.BIL_C, case.src, case.dst
    x0, x1 = K.bil_pair_input(case)
    (a0, v0), (a1, v1) = dense(tuple(x0.shape), DEV, fill=x0), dense(tuple(x1.shape), DEV, fill=x1)
    (b0, o0), (b1, o1) = dense((B, C, Ho, Wo), DEV, out=True), dense((B, C, Ho, Wo), DEV, out=True)
    _run([a0, a1, b0, b1], lambda: L.ts_resize_bilinear_pair_fwd(_ptr(v0), _ptr(v1), _ptr(o0), _ptr(o1), B, C, h, w, Ho, Wo, case.vs[0], case.vs[1], stream))
    _finite(o0, o1)
    for i, (x, o, vs) in enumerate(((x0, o0, 1.0), (x1, o1, 2.5))):
        _exact(case.name, "map%d=single" % i, o, _bilinear(L, stream, x, case.dst, vs, False).cpu())
        _within(case.name, "map%d" % i, K.err_tensor(o, R.resize_bilinear(x.double(), case.dst, vs)), K.bound(case.key, "map%d" % i, K.BASE["out"]))


# ---- search-range candidates -----------------------------------------------------------------------------------------------------
def _range_call(L, stream, case):
    B, (H, W) = K.RANGE_B, case.hw
    d = K.range_input(case)
    (ad, dv), (al, lv), (ah, hv) = dense(tuple(d.shape), DEV, fill=d), dense(tuple(d.shape), DEV, out=True), dense(tuple(d.shape), DEV, out=True)
    ac = Arena(B * case.ctot * H * W, DEV)
    ok = case.coff + 5 <= case.ctot
    cv = ac.carve((B, 5, H, W), (case.ctot * H * W, H * W, W, 1), case.coff * H * W, out=True) if ok else None
    call = lambda: L.ts_range_candidates_fwd(_ptr(dv), _ptr(lv), _ptr(hv), ac.buf.data_ptr() + 4 * GUARD, B, H, W, case.range, case.coff, case.ctot, stream)
    return d, [ad, al, ah, ac], lv, hv, cv, call


@pytest.mark.parametrize("case", K.RANGE, ids=_ids)
def test_range_candidates(case):
    """range < 0 turns low and high round: |high - low| and min(low, high) keep the candidates ascending; the channels beside the five
    written ones stay at the sentinel"""
    L, stream = _api()
    d, arenas, lv, hv, cv, call = _range_call(L, stream, case)
    _run(arenas, call)
    _finite(lv, hv, cv)
    for q, got, ref in zip(("low", "high", "cand"), (lv, hv, cv), R.range_candidates(d.double(), case.range)):
        _within(case.name, q, K.err_tensor(got, ref), K.bound(case.key, q, K.BASE["out"]))
    assert bool((cv[:, 1:] >= cv[:, :-1]).all())


def test_range_candidates_refuses_a_slice_past_the_buffer():
    L, stream = _api()
    d, arenas, lv, hv, cv, call = _range_call(L, stream, K.RangeCase("range_refused", None, (5, 7), 4.0, 4, 8))
    _run(arenas, call, want_rc=K.TS_ERR_SHAPE)
    assert bool((lv == K.SENTINEL).all()) and bool((hv == K.SENTINEL).all()) and bool((arenas[3].buf == K.SENTINEL).all())


# ---- the two softmax upsamplers --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.UPS, ids=_ids)
def test_softmax_upsamplers(case):
    """forward and both gradients through the autograd functions, at non-integer ratios, factors 1 and 3, one-row and one-column maps;
    the x30 logits make the softmax one-hot almost everywhere (the maximum has to be subtracted for that to stay finite)"""
    from temporalstereo_amd import functional as TF
    logits, disp, g = [t.to(DEV) for t in K.up_input(case)]

    def once():
        la, da = logits.clone().requires_grad_(True), disp.clone().requires_grad_(True)
        y = TF.unet_upsample(la, da) if case.kind == "unet" else TF.convex_upsample(la, da, case.dims[2], float(case.dims[2]))
        y.backward(g)
        torch.cuda.synchronize()
        return y.detach(), la.grad, da.grad

    got, again = once(), once()
    _finite(*got)
    for q, a, b, ref, tol in zip(K.UP_QUANTITIES, got, again, K.up_reference(case), K.UP_TOL[case.kind]):
        assert _same_bits(a, b.cpu()), "a second call gives other bits"
        _within(case.name, q, K.err_tol(a, ref, *tol), K.bound(case.key, q, K.BASE["tol"]))
