"""GPU: the train-mode BatchNorm + activation kernels of csrc/batchnorm.hip called on their own through the C ABI, against the
float64 restatement tests/bn_ref.py -- every launch form (one launch, two, three, eval backward), float4 and scalar variants, on
strided and misaligned planes carved out of sentinel-filled buffers (nothing outside the B * C planes may change), and on channels
the convolution-level tests never produce: |mean| >> std, tiny std, constant, an outlier first element, gamma = 40, B * N == 1.

Cases, metric, bounds and the measured fp32 yardstick behind every bound that is not a base bound: tests/bn_cases.py (the table
YARD, pinned by tests/test_batchnorm_ref_cpu.py).  Base bounds, per channel: 5e-6 outputs, 2e-5 gradients, 1e-5 statistics.
"""
import pytest
import torch

import bn_cases as K
import bn_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


class Planes:
    """[B, C, N] planes at `layout` = (offset, bstride, cstride) inside a flat sentinel-filled buffer with GUARD elements of sentinel
    in front of the first and behind the last plane"""

    def __init__(self, shape, layout, fill=None):
        B, C, N = shape
        off, bs, cs = layout
        start = K.GUARD + off
        self.buf = torch.full((start + (B - 1) * bs + (C - 1) * cs + N + K.GUARD,), K.SENTINEL, dtype=torch.float32, device=DEV)
        assert self.buf.data_ptr() % 16 == 0
        self.view = self.buf.as_strided((B, C, N), (bs, cs, 1), start)
        self.bs, self.cs = bs, cs
        inside = torch.zeros_like(self.buf, dtype=torch.bool)
        inside.as_strided((B, C, N), (bs, cs, 1), start).fill_(True)
        self.outside = ~inside
        assert int(inside.sum()) == B * C * N
        if fill is not None:
            self.view.copy_(fill)

    @property
    def ptr(self):
        return self.view.data_ptr()

    def untouched(self):
        return bool((self.buf[self.outside] == K.SENTINEL).all())


def _ptr(t):
    return None if t is None else t.data_ptr()


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


class Run:
    """one case's device tensors and the calls of every form on them"""

    def __init__(self, case):
        from temporalstereo_amd import _lib
        self.lib, self.check, self.stream = _lib.lib(), _lib.check, _lib.current_stream_handle()
        self.case = case
        self.d = K.make_inputs(case)
        B, C, N = case.shape
        self.x = Planes(case.shape, K.layout_of(case, "x"), self.d["x"])
        self.dy = Planes(case.shape, K.layout_of(case, "dy"), self.d["dy"])
        self.gamma, self.beta = _dev(self.d["gamma"]), _dev(self.d["beta"])
        self.ws_bytes = int(self.lib.ts_bn_workspace_bytes(B, C, N))

    def fresh(self):
        B, C, N = self.case.shape
        r = {"out": Planes(self.case.shape, K.layout_of(self.case, "out")), "dx": Planes(self.case.shape, K.layout_of(self.case, "dx")),
             "mean": torch.full((C,), K.SENTINEL, device=DEV), "var": torch.full((C,), K.SENTINEL, device=DEV),
             "s1": torch.full((C,), K.SENTINEL, device=DEV), "s2": torch.full((C,), K.SENTINEL, device=DEV),
             "ws": torch.empty(self.ws_bytes, dtype=torch.uint8, device=DEV), "rm": None, "rv": None, "counter": None}
        assert r["dx"].bs == self.x.bs and r["dx"].cs == self.x.cs
        if self.d["running"] is not None:
            r["rm"], r["rv"] = _dev(self.d["running"][0].clone()), _dev(self.d["running"][1].clone())
            r["counter"] = torch.tensor([41], dtype=torch.int64, device=DEV)
        return r

    def train(self):
        """ts_bn_train_fwd + ts_bn_train_bwd (one launch each below the small bound, two above)"""
        B, C, N = self.case.shape
        c, d, r = self.case, self.d, self.fresh()
        self.check(self.lib.ts_bn_train_fwd(self.x.ptr, _ptr(r["mean"]), _ptr(r["var"]), _ptr(r["rm"]), _ptr(r["rv"]), d["momentum"],
                                            _ptr(r["counter"]), _ptr(self.gamma), _ptr(self.beta), r["out"].ptr, _ptr(r["ws"]), B, C, N,
                                            self.x.bs, self.x.cs, r["out"].bs, r["out"].cs, d["eps"], c.act, self.stream), "ts_bn_train_fwd")
        self.check(self.lib.ts_bn_train_bwd(self.x.ptr, self.dy.ptr, _ptr(r["mean"]), _ptr(r["var"]), _ptr(self.gamma), _ptr(self.beta),
                                            _ptr(r["s1"]), _ptr(r["s2"]), r["dx"].ptr, _ptr(r["ws"]), B, C, N, self.x.bs, self.x.cs,
                                            self.dy.bs, self.dy.cs, d["eps"], c.act, float(B * N), self.stream), "ts_bn_train_bwd")
        torch.cuda.synchronize()
        return r

    def three(self):
        """ts_bn_stats_fwd -> ts_bn_apply_act_fwd and ts_bn_act_bwd_reduce -> ts_bn_act_bwd_apply (the SyncBatchNorm form)"""
        B, C, N = self.case.shape
        c, d, r = self.case, self.d, self.fresh()
        self.check(self.lib.ts_bn_stats_fwd(self.x.ptr, _ptr(r["mean"]), _ptr(r["var"]), _ptr(r["rm"]), _ptr(r["rv"]), d["momentum"],
                                            _ptr(r["counter"]), _ptr(r["ws"]), B, C, N, self.x.bs, self.x.cs, self.stream), "ts_bn_stats_fwd")
        self.check(self.lib.ts_bn_apply_act_fwd(self.x.ptr, _ptr(r["mean"]), _ptr(r["var"]), _ptr(self.gamma), _ptr(self.beta), r["out"].ptr,
                                                B, C, N, self.x.bs, self.x.cs, r["out"].bs, r["out"].cs, d["eps"], c.act, self.stream),
                   "ts_bn_apply_act_fwd")
        self.check(self.lib.ts_bn_act_bwd_reduce(self.x.ptr, self.dy.ptr, _ptr(r["mean"]), _ptr(r["var"]), _ptr(self.gamma), _ptr(self.beta),
                                                 _ptr(r["s1"]), _ptr(r["s2"]), _ptr(r["ws"]), B, C, N, self.x.bs, self.x.cs, self.dy.bs,
                                                 self.dy.cs, d["eps"], c.act, self.stream), "ts_bn_act_bwd_reduce")
        self.check(self.lib.ts_bn_act_bwd_apply(self.x.ptr, self.dy.ptr, _ptr(r["mean"]), _ptr(r["var"]), _ptr(self.gamma), _ptr(self.beta),
                                                _ptr(r["s1"]), _ptr(r["s2"]), r["dx"].ptr, B, C, N, self.x.bs, self.x.cs, self.dy.bs,
                                                self.dy.cs, d["eps"], c.act, 1, float(B * N), self.stream), "ts_bn_act_bwd_apply")
        torch.cuda.synchronize()
        return r


def _assert_close(case, r, ref, d, form):
    B, C, N = case.shape
    kinds = K.case_kinds(case)
    bnd = K.bounds(case)
    assert r["out"].untouched(), "%s %s: out written outside its planes" % (case.name, form)
    assert r["dx"].untouched(), "%s %s: dx written outside its planes" % (case.name, form)
    got = {k: (r[k].view if k in ("out", "dx") else r[k]) for k in ("out", "dx", "s1", "s2")}
    assert all(bool(torch.isfinite(v).all()) for v in got.values()), "%s %s: non-finite result" % (case.name, form)
    e = K.errors(got, ref)
    sm, sv, srm, srv = K.stat_scales(ref["mean"], ref["var"], B * N, d["running"])
    figures = [("out", e["out"], bnd["out"]), ("dx", e["dx"], bnd["dx"]), ("s1", e["s1"], bnd["s"]), ("s2", e["s2"], bnd["s"]),
               ("mean", K.err_vec(r["mean"], ref["mean"], sm), K.BASE["stat"]), ("var", K.err_vec(r["var"], ref["var"], sv), K.BASE["stat"])]
    if d["running"] is not None:
        figures += [("running_mean", K.err_vec(r["rm"], ref["running"][0], srm), K.BASE["stat"]),
                    ("running_var", K.err_vec(r["rv"], ref["running"][1], srv), K.BASE["stat"])]
        assert int(r["counter"]) == 42, "%s %s: num_batches_tracked %d after one call from 41" % (case.name, form, int(r["counter"]))
    bad = []
    for name, err, bound in figures:
        bound = torch.as_tensor(bound, dtype=torch.float64).expand(C)
        for c in range(C) if C <= 8 else [int(i) for i in torch.nonzero(err > bound).flatten()[:8]]:
            line = "%s %s %-12s channel %d (%s): %.3g (bound %.3g)" % (case.name, form, name, c, kinds[c], float(err[c]), float(bound[c]))
            if C <= 8:
                print(line)
            if not float(err[c]) <= float(bound[c]):
                bad.append(line)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("case", K.CASES, ids=[c.name for c in K.CASES])
def test_train_forms_against_float64(case):
    """ts_bn_train_{fwd,bwd} in the form the case names -- and for the two-launch cases the three-launch form beside it, which must
    give the same bits -- against bn_ref: out, mean, var, running statistics, s1, s2, dx within the bounds of bn_cases, the counter
    advanced by exactly one, nothing written outside the planes."""
    from temporalstereo_amd import _lib
    d = K.make_inputs(case)
    ref = K.reference(case, d)
    old = _lib.lib().ts_bn_set_small_elems(0 if case.form == "two" else -1)
    try:
        run = Run(case)
        r = run.train()
        _assert_close(case, r, ref, d, "train")
        assert run.x.untouched() and run.dy.untouched()
        B, N = case.shape[0], case.shape[2]
        if case.form == "two" or B * N > old:
            t = run.three()
            _assert_close(case, t, ref, d, "three-launch")
            for k in ("mean", "var", "s1", "s2", "rm", "rv", "counter"):
                assert (r[k] is None and t[k] is None) or torch.equal(r[k], t[k]), "%s: %s differs between the two- and the three-launch form" % (case.name, k)
            for k in ("out", "dx"):
                assert torch.equal(r[k].buf, t[k].buf), "%s: %s differs between the two- and the three-launch form" % (case.name, k)
    finally:
        _lib.lib().ts_bn_set_small_elems(old)


@pytest.mark.parametrize("form", ["small", "two", "three"])
def test_counter_advances_by_one_per_call(form):
    """num_batches_tracked after three calls of each form: exactly three more"""
    from temporalstereo_amd import _lib
    case = next(c for c in K.CASES if c.form == ("small" if form == "small" else "two") and c.running)
    old = _lib.lib().ts_bn_set_small_elems(-1 if form == "small" else 0)
    try:
        run = Run(case)
        B, C, N = case.shape
        r = run.fresh()
        for i in range(3):
            if form == "three":
                rc = run.lib.ts_bn_stats_fwd(run.x.ptr, _ptr(r["mean"]), _ptr(r["var"]), _ptr(r["rm"]), _ptr(r["rv"]), 0.1, _ptr(r["counter"]),
                                             _ptr(r["ws"]), B, C, N, run.x.bs, run.x.cs, run.stream)
            else:
                rc = run.lib.ts_bn_train_fwd(run.x.ptr, _ptr(r["mean"]), _ptr(r["var"]), _ptr(r["rm"]), _ptr(r["rv"]), 0.1, _ptr(r["counter"]),
                                             _ptr(run.gamma), _ptr(run.beta), r["out"].ptr, _ptr(r["ws"]), B, C, N, run.x.bs, run.x.cs,
                                             r["out"].bs, r["out"].cs, run.d["eps"], case.act, run.stream)
            run.check(rc, form)
            assert int(r["counter"]) == 42 + i
    finally:
        _lib.lib().ts_bn_set_small_elems(old)


@pytest.mark.parametrize("case", K.EVAL_CASES, ids=[c.name for c in K.EVAL_CASES])
def test_eval_forward_and_backward_on_given_statistics(case):
    """ts_bn_apply_act_fwd and ts_bn_act_bwd_apply(train = 0) on arbitrary mean / var (null sums): base bounds, every channel being
    well-conditioned (tests/test_batchnorm_ref_cpu.py checks that 4 x the fp32 yardstick of these inputs is below them)."""
    from temporalstereo_amd import _lib
    L, stream = _lib.lib(), _lib.current_stream_handle()
    B, C, N = case.shape
    d = K.eval_inputs(case)
    x, dy = Planes(case.shape, K.layout_of(case, "x"), d["x"]), Planes(case.shape, K.layout_of(case, "dy"), d["dy"])
    out, dx = Planes(case.shape, K.layout_of(case, "out")), Planes(case.shape, K.layout_of(case, "dx"))
    mean, var, gamma, beta = _dev(d["mean"]), _dev(d["var"]), _dev(d["gamma"]), _dev(d["beta"])
    _lib.check(L.ts_bn_apply_act_fwd(x.ptr, _ptr(mean), _ptr(var), _ptr(gamma), _ptr(beta), out.ptr, B, C, N, x.bs, x.cs, out.bs, out.cs,
                                     d["eps"], case.act, stream), "ts_bn_apply_act_fwd")
    _lib.check(L.ts_bn_act_bwd_apply(x.ptr, dy.ptr, _ptr(mean), _ptr(var), _ptr(gamma), _ptr(beta), None, None, dx.ptr, B, C, N, x.bs, x.cs,
                                     dy.bs, dy.cs, d["eps"], case.act, 0, 0.0, stream), "ts_bn_act_bwd_apply")
    torch.cuda.synchronize()
    assert out.untouched() and dx.untouched() and x.untouched() and dy.untouched()
    ro = bn_ref.bn_act_fwd(d["x"], d["gamma"], d["beta"], d["eps"], case.act, mean=d["mean"], var=d["var"])[0]
    rdx = bn_ref.bn_act_bwd(d["x"], d["dy"], d["mean"], d["var"], d["gamma"], d["beta"], d["eps"], case.act, False, B * N)[0]
    eo, ed = K.err_planes(out.view, ro), K.err_planes(dx.view, rdx)
    print(case.name, "out", eo.tolist(), "dx", ed.tolist())
    assert float(eo.max()) <= K.BASE["out"] and float(ed.max()) <= K.BASE["grad"]


# ---- ts_bn_sync_merge ------------------------------------------------------------------------------------------------------------
def run_merge(recs, C, momentum, running):
    from temporalstereo_amd import _lib
    gathered = torch.cat([torch.cat([m, v, torch.tensor([n])]) for m, v, n in recs]).float().to(DEV)
    mean, var = torch.full((C + 64,), K.SENTINEL, device=DEV), torch.full((C + 64,), K.SENTINEL, device=DEV)
    inv = torch.full((1,), K.SENTINEL, device=DEV)
    rm, rv = (None, None) if running is None else (_dev(running[0].clone()), _dev(running[1].clone()))
    _lib.check(_lib.lib().ts_bn_sync_merge(_ptr(gathered), len(recs), C, _ptr(mean), _ptr(var), _ptr(rm), _ptr(rv), momentum, _ptr(inv),
                                           _lib.current_stream_handle()), "ts_bn_sync_merge")
    torch.cuda.synchronize()
    assert bool((mean[C:] == K.SENTINEL).all()) and bool((var[C:] == K.SENTINEL).all())
    return mean[:C], var[:C], rm, rv, inv


@pytest.mark.parametrize("running", [True, False])
@pytest.mark.parametrize("C", [1, 64, 65, 130])
@pytest.mark.parametrize("world", [1, 2, 3, 5])
def test_sync_merge_against_float64(world, C, running):
    import synth
    recs = K.merge_records(world, C)
    run0 = (torch.from_numpy(synth.normal(310, "rm", (C,), 0.2)), torch.from_numpy(synth.uniform(310, "rv", (C,), 0.5, 1.5))) if running else None
    momentum = 0.1
    mean, var, rm, rv, inv = run_merge(recs, C, momentum, run0)
    rmean, rvar, rrun, rinv = bn_ref.sync_merge(recs, momentum, run0)
    n = 1.0 / rinv
    sm, sv, srm, srv = K.stat_scales(rmean, rvar, n, run0)
    assert float(K.err_vec(mean, rmean, sm).max()) <= K.BASE["stat"]
    assert float(K.err_vec(var, rvar, sv).max()) <= K.BASE["stat"]
    assert abs(float(inv) - rinv) <= 1e-7 * rinv
    if running:
        assert float(K.err_vec(rm, rrun[0], srm).max()) <= K.BASE["stat"]
        assert float(K.err_vec(rv, rrun[1], srv).max()) <= K.BASE["stat"]


def test_sync_merge_of_parts_equals_the_statistics_of_the_whole():
    """three ranks' ts_bn_stats_fwd records, merged, against ts_bn_stats_fwd on the concatenated batch (and both against float64)"""
    from temporalstereo_amd import _lib
    import synth
    L, stream = _lib.lib(), _lib.current_stream_handle()
    C, N, parts = 5, 405, (1, 3, 2)
    kinds = ("n01", "n31", "wide", "m50", "tiny")
    x = K.channel_data(320, "x", kinds, sum(parts), N)
    for c in range(C):                       # the ranks see different data: shift each rank's share by a few std
        x[1:4, c] += 3.0 * K.KINDS[kinds[c]][1]
        x[4:, c] -= 2.0 * K.KINDS[kinds[c]][1]

    def stats(t):
        B = t.shape[0]
        t = t.to(DEV).contiguous()
        mean, var = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
        ws = torch.empty(int(L.ts_bn_workspace_bytes(B, C, N)), dtype=torch.uint8, device=DEV)
        _lib.check(L.ts_bn_stats_fwd(_ptr(t), _ptr(mean), _ptr(var), None, None, 0.1, None, _ptr(ws), B, C, N, C * N, N, stream), "ts_bn_stats_fwd")
        torch.cuda.synchronize()
        return mean.cpu(), var.cpu()

    recs, b0 = [], 0
    for b in parts:
        m, v = stats(x[b0:b0 + b])
        recs.append((m, v, float(b * N)))
        b0 += b
    mean, var, _, _, inv = run_merge(recs, C, 0.1, None)
    wmean, wvar = stats(x)
    rmean, rvar = bn_ref.batch_stats(x)
    sm, sv, _, _ = K.stat_scales(rmean, rvar, sum(parts) * N, None)
    for got_m, got_v in ((mean, var), (wmean, wvar)):
        assert float(K.err_vec(got_m, rmean, sm).max()) <= K.BASE["stat"]
        assert float(K.err_vec(got_v, rvar, sv).max()) <= K.BASE["stat"]
    assert abs(float(inv) * sum(parts) * N - 1.0) <= 1e-6


# ---- ts_channel_sum_fwd ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 2, 16384), (2, 2, 16385), (1, 2, 32768), (1, 2, 32769), (3, 2, 77)])
def test_channel_sum_on_padded_strides(shape):
    """both forms of ts_channel_sum_fwd (B * N on either side of its 32768 switch) on planes with padded strides: the sum against
    float64 (2e-7 of sum |x|, the bound of test_channel_sum_both_forms), the gaps ignored (a sentinel read would show at once)"""
    from temporalstereo_amd import _lib
    import synth
    B, C, N = shape
    L = _lib.lib()
    xv = torch.from_numpy(synth.normal(330, "cs", shape))
    x = Planes(shape, (0, C * (N + 8) + 16, N + 8), xv)
    out = torch.full((C + 64,), K.SENTINEL, device=DEV)
    ws = torch.empty(int(L.ts_bn_workspace_bytes(B, C, N)), dtype=torch.uint8, device=DEV)
    _lib.check(L.ts_channel_sum_fwd(x.ptr, _ptr(out), _ptr(ws), B, C, N, x.bs, x.cs, _lib.current_stream_handle()), "ts_channel_sum_fwd")
    torch.cuda.synchronize()
    assert x.untouched() and bool((out[C:] == K.SENTINEL).all())
    want = xv.double().sum(dim=(0, 2))
    scale = float(xv.double().abs().sum(dim=(0, 2)).max())
    assert float((out[:C].double().cpu() - want).abs().max()) <= 2e-7 * scale
