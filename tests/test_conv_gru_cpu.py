"""ConvGRU without a GPU: tests/conv_gru_ref.py (the plain-torch restatement, the fp64 yardstick of tests/test_conv_gru_gpu.py) and
temporalstereo_amd.ConvGRU on CPU tensors against the reference's own runs in tests/golden/conv_gru_*.npz (tools/gen_golden.py
--only-convgru); the constructor and state-dict contract; the argument checks of the new C-ABI entries (they come before any launch).

Bars: the fixture's recorded deviation of the reference's fp32 run from its fp64 run.  conv_gru_ref in fp64 stands where the reference's
fp64 run stands (1e-10, asserted by the generator), so it lies within dev_* (+ 1e-9) of the stored fp32 values; conv_gru_ref in fp32 is
the reference's own op sequence and lies within dev_* of them too.  Gradients: relative L2 <= rel_grad_* (+ 1e-9) where the whole array is
stored.  Where 8192 seeded positions of a larger array are stored the same ratio is formed over those positions while rel_grad_* was
formed over the whole array: a mean of 8192 squared errors scatters around the whole array's by ~sqrt(2 / 8192) = 1.6 % (a chi-square
of that many terms), its root by half of that, and 1.25 leaves that thirty-fold.
"""
import ctypes

import pytest
import torch

import conv_gru_ref as R
from compare import T, err, null_sweep, rel_l2
import temporalstereo_amd as ts
from temporalstereo_amd import _lib
from temporalstereo_amd import functional as TF

FIXTURES = ("a", "b", "c", "d")


@pytest.mark.parametrize("tag", FIXTURES)
def test_ref_reproduces_the_fixture(tag):
    g = R.load_fixture(tag)
    backward = "grad_h" in g
    assert tuple(g["keys"]) == R.KEYS
    for dt in (torch.float64, torch.float32):
        run = R.run(g["seed"], g["shape"], dt, backward)
        for k in R.STAGES + ("out3",):
            assert err(R.sample(run[k], g["seed"]), T(g[k])) <= float(g["dev_" + k]) + 1e-9, (tag, dt, k)
        if not backward:
            continue
        r64 = run if dt is torch.float64 else R.run(g["seed"], g["shape"], torch.float64)
        for k in ("h", "x") + R.KEYS:
            got, ref, want = R.sample(run["grad_" + k], g["seed"]), R.sample(r64["grad_" + k], g["seed"]), T(g["grad_" + k])
            slack = 1.0 if R.sample_index(g["seed"], run["grad_" + k].numel()) is None else 1.25
            assert rel_l2(got, want, ref) <= slack * float(g["rel_grad_" + k]) + 1e-9, (tag, dt, k)


@pytest.mark.parametrize("tag", FIXTURES)
def test_module_on_cpu_is_the_restatement(tag):
    """CPU tensors take the reference's op sequence: the same operators in the same order as conv_gru_ref, so the same bits."""
    g = R.load_fixture(tag)
    B, Ch, Cx, H, W = g["shape"]
    m = ts.ConvGRU(Cx, Ch)
    m.load_state_dict(R.fixture_state(g["seed"], Ch, Cx), strict=True)
    h, x = R.fixture_input(g["seed"], g["shape"])
    with torch.no_grad():
        out = m(h, x)
        want = R.conv_gru(h, x, R.fixture_state(g["seed"], Ch, Cx))["out"]
        assert torch.equal(out, want)
        assert err(R.sample(out, g["seed"]), T(g["out"])) <= float(g["dev_out"]) + 1e-9
        assert torch.equal(m._reference_forward(h, x), out)
        m64 = m.double()
        assert err(m64(h.double(), x.double()), out) <= float(g["dev_out"]) + 1e-9            # another dtype: the same path


def test_constructor_contract():
    m = ts.ConvGRU(5, 12)
    assert (m.in_planes, m.hidden_planes) == (5, 12)
    assert list(m.state_dict().keys()) == list(R.KEYS)
    for name in ("convz", "convr", "convq"):
        conv = getattr(m, name)
        assert isinstance(conv, torch.nn.Conv2d)
        assert tuple(conv.weight.shape) == (12, 17, 3, 3) and tuple(conv.bias.shape) == (12,)
        assert conv.padding == (1, 1) and conv.stride == (1, 1)
    state = R.fixture_state(7, 12, 5)
    res = m.load_state_dict(state, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in m.state_dict().items():
        assert torch.equal(v, state[k])
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in state.items() if k != "convq.bias"}, strict=True)
    assert ts.ConvGRU is ts.recurrent.ConvGRU and ts.conv_gru is TF.conv_gru


def test_functional_refuses_cpu_tensors():
    state = R.fixture_state(7, 12, 5)
    h, x = R.fixture_input(7, (1, 12, 5, 4, 6))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        TF.conv_gru(h, x, *[state[k] for k in R.KEYS])
    assert TF.conv_gru_supported(64, 64) and TF.conv_gru_supported(1, 1)
    assert not TF.conv_gru_supported(65, 8) and not TF.conv_gru_supported(8, 65) and not TF.conv_gru_supported(0, 8)


def test_abi_version_and_argument_checks():
    L = _lib.lib()
    assert L.ts_version() >= 19
    buf = ctypes.create_string_buffer(64)
    one = (ctypes.addressof(buf) + 15) // 16 * 16        # never dereferenced by a call that is refused; 16-byte aligned
    big = 1 << 20
    N = 6 * 7

    # ts_conv_gru_weight_bytes / ts_conv_gru_weight_layout(wz, wr, wq, w_l, Ch, Cx, stream)
    assert L.ts_conv_gru_weight_bytes(12, 5) > 0 and L.ts_conv_gru_weight_bytes(64, 64) >= 3 * 64 * 128 * 9 * 4
    assert L.ts_conv_gru_weight_bytes(65, 8) == 0 and L.ts_conv_gru_weight_bytes(8, 65) == 0 and L.ts_conv_gru_weight_bytes(0, 8) == 0
    null_sweep(L.ts_conv_gru_weight_layout, (one, one, one, one, 12, 5, None), (0, 1, 2, 3), "weight_layout")
    assert L.ts_conv_gru_weight_layout(one, one, one, one, 0, 5, None) == -2
    assert L.ts_conv_gru_weight_layout(one, one, one, one, 12, -1, None) == -2
    assert L.ts_conv_gru_weight_layout(one, one, one, one, 65, 5, None) == -3
    assert L.ts_conv_gru_weight_layout(one, one, one, one, 12, 65, None) == -3

    # ts_conv_gru_gates_fwd(h, x, w_l, bz, br, z, rh, r, B, Ch, Cx, H, W, h_bs, h_cs, x_bs, x_cs, stream): r may be NULL
    # ts_conv_gru_out_fwd(rh, x, w_l, bq, z, h, out, q, B, Ch, Cx, H, W, h_bs, h_cs, x_bs, x_cs, stream): q may be NULL
    for fn, what in ((L.ts_conv_gru_gates_fwd, "gates_fwd"), (L.ts_conv_gru_out_fwd, "out_fwd")):
        ok = lambda B=2, Ch=12, Cx=5, H=6, W=7, hb=12 * N, hc=N, xb=5 * N, xc=N: \
            (one,) * 8 + (B, Ch, Cx, H, W, hb, hc, xb, xc, None)
        null_sweep(fn, ok(), (0, 1, 2, 3, 4, 5, 6), what)
        # r / q may be NULL: with it the call gets past the pointer checks, to the alignment check of w_l that follows them
        a = list(ok())
        a[7], a[2] = None, one + 4
        assert fn(*a) == -4, what
        for bad in (dict(B=0), dict(Ch=0), dict(Cx=-3), dict(H=0), dict(W=0)):
            assert fn(*ok(**bad)) == -2, (what, bad)
        assert fn(*ok(hc=N - 1)) == -2 and b"overlap" in L.ts_last_error_string()          # channels of h overlap
        assert fn(*ok(hb=12 * N - 1)) == -2                                                  # batch items of h overlap
        assert fn(*ok(xc=N - 1)) == -2 and fn(*ok(xb=5 * N - 1)) == -2
        assert fn(*ok(Ch=65, hb=65 * N)) == -3 and fn(*ok(Cx=65, xb=65 * N)) == -3
        assert fn(*ok(B=1, H=big, hc=big * 7, xc=big * 7)) == -3 and fn(*ok(B=1, W=big, hc=big * 6, xc=big * 6)) == -3

    # ts_conv_gru_gate_bwd_a(dout, z, q, h, dq_pre, dz_pre, dh, B, Ch, N, h_bs, h_cs, dz_bs, dz_cs, stream)
    ok = lambda B=2, Ch=12, n=N, hb=12 * N, hc=N, zb=24 * N, zc=N: (one,) * 7 + (B, Ch, n, hb, hc, zb, zc, None)
    fn = L.ts_conv_gru_gate_bwd_a
    null_sweep(fn, ok(), tuple(range(7)), "gate_bwd_a")
    assert fn(*ok(B=0)) == -2 and fn(*ok(Ch=0)) == -2 and fn(*ok(n=0)) == -2
    assert fn(*ok(hc=N - 1)) == -2 and fn(*ok(zc=N - 1)) == -2 and fn(*ok(zb=12 * N - 1)) == -2
    assert fn(*ok(Ch=65, hb=65 * N, zb=130 * N)) == -3
    assert fn(*ok(B=1, n=1 << 40, hc=1 << 40, zc=1 << 40)) == -3

    # ts_conv_gru_gate_bwd_b(d_rh, r, h, dr_pre, dh, B, Ch, N, drh_bs, drh_cs, h_bs, h_cs, dr_bs, dr_cs, stream)
    ok = lambda B=2, Ch=12, n=N, gb=17 * N, gc=N, hb=12 * N, hc=N, rb=24 * N, rc=N: (one,) * 5 + (B, Ch, n, gb, gc, hb, hc, rb, rc, None)
    fn = L.ts_conv_gru_gate_bwd_b
    null_sweep(fn, ok(), tuple(range(5)), "gate_bwd_b")
    assert fn(*ok(B=0)) == -2 and fn(*ok(Ch=-1)) == -2 and fn(*ok(n=0)) == -2
    assert fn(*ok(gc=N - 1)) == -2 and fn(*ok(hc=N - 1)) == -2 and fn(*ok(rc=N - 1)) == -2 and fn(*ok(gb=12 * N - 1)) == -2
    assert fn(*ok(Ch=65, gb=70 * N, hb=65 * N, rb=130 * N)) == -3
    assert fn(*ok(B=1, n=1 << 40, gc=1 << 40, hc=1 << 40, rc=1 << 40)) == -3

    # ts_conv_gru_grad_sum(dcat_g, dcat_q, dh, dx, B, Ch, Cx, N, stream): dx may be NULL
    ok = lambda B=2, Ch=12, Cx=5, n=N: (one,) * 4 + (B, Ch, Cx, n, None)
    fn = L.ts_conv_gru_grad_sum
    null_sweep(fn, ok(), (0, 1, 2), "grad_sum")              # (dx = NULL is exercised on the device: x without a gradient)
    assert fn(*ok(B=0)) == -2 and fn(*ok(Ch=0)) == -2 and fn(*ok(Cx=0)) == -2 and fn(*ok(n=-1)) == -2
    assert fn(*ok(Ch=65)) == -3 and fn(*ok(Cx=65)) == -3 and fn(*ok(B=1, n=1 << 40)) == -3
