"""CPU: the plain restatement tests/block_cost_ref.py pinned to the oracle (itself pinned to reference-made goldens) in float64, to
closed forms, and the fp32 position sequence to the float64 position; the launch-form table and the transition list of
tests/block_cost_cases.py pinned to its restatement of launch_fwd / launch_bwd.  `-s` prints the figures."""
import pytest
import torch

import block_cost_cases as K
import block_cost_ref as R
import oracle
import synth

F64 = torch.float64


def _maps(seed, B, C, H, W, D, lo=-3.0, hi=None):
    t = lambda a: torch.from_numpy(a).double()
    hi = W + 3.0 if hi is None else hi
    return t(synth.normal(seed, "L", (B, C, H, W))), t(synth.normal(seed, "R", (B, C, H, W))), t(synth.uniform(seed, "d", (B, D, H, W), lo, hi))


# H, W over 4..9 (pooled axes of size 1 and 2), D = 2 and more, scales 1..3, more than one group and batch item
PIN = [(1, 8, h, w, 2, 3) for h in range(4, 10) for w in (4, 5, 7, 8, 9)] + \
      [(2, 16, 5, 6, 3, 1), (1, 8, 9, 4, 2, 1), (1, 16, 6, 9, 4, 2), (2, 8, 7, 7, 2, 2), (1, 8, 12, 21, 5, 3), (1, 24, 9, 16, 3, 3), (1, 8, 4, 37, 7, 3)]


@pytest.mark.parametrize("shape", PIN, ids=lambda s: "x".join(map(str, s)))
def test_restatement_is_the_oracle_in_float64(shape):
    """outputs and autograd gradients of both paths; the oracle's y and z coordinate round trips vanish in float64"""
    B, C, H, W, D, scales = shape
    worst = 0.0
    for sampled in (False, True):
        L, Rt, d = _maps(1200 + H * W, B, C, H, W, D)
        d[:, 0] = torch.round(d[:, 0])
        outs, grads = [], []
        for fn in (R.block_cost, oracle.block_cost):
            ins = [L.clone().requires_grad_(), Rt.clone().requires_grad_()] + ([d.clone().requires_grad_()] if sampled else [])
            out = fn(ins[0], ins[1], ins[2] if sampled else D, scales)
            g = torch.from_numpy(synth.normal(7, "g", tuple(out.shape))).double()
            outs.append(out.detach())
            grads.append(torch.autograd.grad(out, ins, g))
        assert outs[0].shape == outs[1].shape
        worst = max([worst, K.err_planes(outs[0], outs[1])] + [K.err_tensor(a, b) for a, b in zip(*grads)])
    print("%s  restatement vs oracle (float64, outputs and gradients): %.3g" % (shape, worst))
    assert worst <= 1e-12


def test_zero_candidates_give_the_right_map():
    """(to the rounding of the coordinate round trip, which is not exactly the identity: a tap lands an ulp of the position beside its
    column, so the error is that times the step between neighbouring columns, at most twice the plane's maximum)"""
    L, Rt, d = _maps(3, 2, 8, 6, 11, 3)
    for pos_dtype in (F64, torch.float32):
        out = R.block_cost(L, Rt, torch.zeros_like(d), 3, pos_dtype=pos_dtype)
        err = K.err_planes(out[:, 8:16], Rt.unsqueeze(2).expand(2, 8, 3, 6, 11))
        print("disp = 0, position in %s: warped half vs right map %.3g" % (pos_dtype, err))
        assert err <= 2 * 3 * 8 * float(torch.finfo(pos_dtype).eps)              # 3 ulp(W) of the position test below, ulp(11) = 8 eps
        assert torch.equal(out[:, :8], L.unsqueeze(2).expand(2, 8, 3, 6, 11))


def test_integer_candidates_give_the_int_path():
    B, C, H, W, D = 1, 16, 7, 13, 6
    L, Rt, _ = _maps(4, B, C, H, W, D)
    d = torch.arange(D, dtype=F64).view(1, D, 1, 1).expand(B, D, H, W)
    s, i = R.block_cost(L, Rt, d, 3), R.block_cost(L, Rt, D, 3)
    errs = (K.err_planes(s[:, C:2 * C], R.shift_taps(Rt, D)), K.err_planes(-(s[:, :C] - s[:, C:2 * C]) ** 2, i[:, :C]), K.err_planes(s[:, 2 * C:], i[:, C:]))
    print("integer candidates vs the int path (float64; warped half, main channels, correlation blocks): %.3g %.3g %.3g" % errs)
    assert max(errs) <= 1e-13                                                    # the round trip again: a few float64 ulp of W = 13


@pytest.mark.parametrize("pos_dtype", [F64, torch.float32])
def test_far_candidates_give_exact_zeros(pos_dtype):
    B, C, H, W = 1, 8, 5, 9
    L, Rt, _ = _maps(5, B, C, H, W, 2)
    mags = [W + 2.0, W + 2.5, 1e3, 1e6, 3e9]
    d = torch.tensor([s * m for m in mags for s in (1.0, -1.0)], dtype=F64).view(1, -1, 1, 1).expand(B, 2 * len(mags), H, W)
    out = R.block_cost(L, Rt, d, 3, pos_dtype=pos_dtype)
    assert bool((out[:, C:2 * C] == 0).all()) and bool(torch.isfinite(out).all())
    assert torch.equal(R.block_cost(L, Rt, K.candidates(0, B, 6, H, W, "far").double(), 3, pos_dtype=pos_dtype)[:, C:2 * C], torch.zeros(B, C, 6, H, W, dtype=F64))


def test_a_one_by_one_quarter_map_expands_to_a_constant():
    B, C, H, W, D = 2, 8, 4, 4, 3
    L, Rt, d = _maps(6, B, C, H, W, D)
    out = R.block_cost(L, Rt, d, 3)
    q = out[:, 2 * C + 2]                                                       # [B, D, H, W]: the 1/4 map's block, one group
    assert torch.equal(q, q[..., :1, :1].expand_as(q))
    e = (L.unsqueeze(2) - out[:, C:2 * C]).mean((3, 4))                         # [B, C, D]
    assert K.err_tensor(q[..., 0, 0], -(e * e).sum(1)) <= 1e-14
    for h, w in ((4, 7), (7, 4), (5, 9)):                                       # one pooled axis of size 1: constant along it
        L, Rt, d = _maps(6, B, C, h, w, D)
        q = R.block_cost(L, Rt, d, 3)[:, 2 * C + 2]
        if h < 8:
            assert torch.equal(q, q[..., :1, :].expand_as(q))
        if w < 8:
            assert torch.equal(q, q[..., :, :1].expand_as(q))


def test_fp32_position_is_the_float64_position_to_a_few_ulp_of_the_width():
    for W in (4, 37, 136, 256, 600, 676):
        d = torch.from_numpy(synth.uniform(8, "d", (1, 64, 5, W), -3.0, W + 3.0))
        d[:, 0] = torch.round(d[:, 0])
        p32, p64 = R.source_position(d, W, torch.float32), R.source_position(d.double(), W, F64)
        ulp = float(torch.finfo(torch.float32).eps) * 2.0 ** torch.floor(torch.log2(torch.tensor(float(W)))).item()
        err = float((p32.double() - p64).abs().max())
        print("W = %4d: |fp32 position - float64 position| <= %.3g = %.2f ulp(W)" % (W, err, err / ulp))
        # xs / (W-1) rounds to half an ulp of a value up to 1 + 6 / W, the subtraction and the addition of 1 to half an ulp of up to 2 each
        # (in position units: times (W-1) / 2), the final product to half an ulp of W: under 3 ulp(W) together
        assert err <= 3.0 * ulp
        assert float((R.source_position(d.double(), W, F64) - (torch.arange(W, dtype=F64) - d.double())).abs().max()) <= 1e-12 * W


def test_form_table_and_transitions_are_the_restated_launch_rules():
    doc = K.__doc__.split("FORM TABLE BEGIN\n")[1].split("\nFORM TABLE END")[0]
    assert doc == K.form_table()
    assert list(K.TRANSITIONS) == K.derive_transitions()
    for w, D in zip(K.PASS_STEPS, (16, 17)):
        assert K.fwd_form("sampled", w, D) != K.fwd_form("sampled", w - 4, D) and K._family(K.fwd_form("sampled", w, D)) == K._family(K.fwd_form("sampled", w - 4, D))
    assert len({c.name for c in K.FWD + K.BWD + K.MANY_PLANES}) == len(K.FWD + K.BWD + K.MANY_PLANES)
    assert all(K.adjoint_form(c.B, c.C, c.H, c.W, c.D, c.scales) == "adjoint_generic" for c in K.MANY_PLANES)
    assert len(K.NULLS) == 8 and len(K.GRADS_OFF) == 7
    assert K.bwd_form("sampled", 40, 3, grads_aligned=False) == "bwd_tile<scalar>" and K.bwd_form("int", 132, 17, grads_aligned=False) == "bwd_main<vec,staged>"


def test_every_form_of_the_table_is_a_case():
    """the forms no earlier direct test ran -- fast<vec,8>, bwd_rows past 64 KB of LDS, bwd_tile at 512 lanes, the non-monotonic corner
    of D = 5 -- and every other form the rules can produce up to the widest case"""
    run_f = {K.fwd_form(e, c.W, c.D, c.aligned) for c in K.FWD for e in K.FWD_ENTRIES}
    run_b = {K.bwd_form(e, c.W, c.D, c.aligned) for c in K.BWD for e in K.BWD_ENTRIES}
    for f in ("fast<vec,8>", "fast<vec,2>", "fast<vec,3>", "fast<vec,4>", "fast<scalar,2>", "fast<scalar,4>", "fast<scalar,8>", "main<vec>", "main<scalar>",
              "corr_rows<1,256>", "corr_rows<2,256>", "corr_rows<2,512>"):
        assert f in run_f, f
    for f in ("bwd_rows<256>", "bwd_rows<256> lds>64K", "bwd_rows<512> lds>64K", "bwd_tile<vec>", "bwd_tile<scalar>", "bwd_main<vec,staged>",
              "bwd_main<scalar,staged>", "bwd_main<vec,unstaged>", "bwd_main<scalar,unstaged>"):
        assert f in run_b, f
    assert K.bwd_form("sampled", 128, 16, False, lanes=True) == "bwd_tile<scalar>@512" and K.bwd_form("int", 128, 16, True, lanes=True) == "bwd_tile<vec>@512"
    assert K.fwd_form("sampled", 256, 5) == "main<vec>" and K.fwd_form("sampled", 260, 5) == "fast<vec,3>"
    lanes = {K.fwd_form(e, c.W, c.D, c.aligned, lanes=True).split("@")[1] for c in K.FWD for e in ("sampled",) if K.fwd_form(e, c.W, c.D, c.aligned).startswith("fast")}
    assert lanes == {str(n) for n in range(64, 513, 64)}
