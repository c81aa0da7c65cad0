"""Split-input entries (include/ts_hip.h: ts_*_split_fwd): an input whose channels [0, Csplit) and [Csplit, Cin) live in two
allocations is read in place.  The kernels, their chunk order and their arithmetic are those of the plain entries, so every result
is held to BIT equality (torch.equal) with the plain entry on torch.cat([a, b], 1) -- never to a tolerance.

The two parts of every input sit directly between runs of NaN (and, with a batch stride longer than the channels, with NaN between
the batch items), the last channel of `a` and the first of `b` hold +-1e30 under zero weights: a halo or seam read that leaves its
allocation, or a channel index off by one at the seam, cannot cancel out."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    for _p in (ROOT, os.path.join(ROOT, "tests")):
        if _p not in sys.path:
            sys.path.insert(0, _p)

pytestmark = pytest.mark.gpu

NAN = float("nan")
FENCE = 64                      # floats of NaN on either side of a part (a multiple of 4: the parts stay 16-byte aligned)
UNSUPPORTED = -3                # TS_ERR_UNSUPPORTED


def _dev():
    return torch.device("cuda:0")


def _fenced(values, extra_channels=0):
    """A copy of `values` [B, C, ...] as a view with batch stride (C + extra_channels) planes into a buffer that is NaN everywhere else."""
    B, C = values.shape[:2]
    rest = tuple(values.shape[2:])
    plane = 1
    for n in rest:
        plane *= n
    n = B * (C + extra_channels) * plane
    buf = torch.full((FENCE + n + FENCE,), NAN, device=values.device)
    view = buf[FENCE:FENCE + n].view((B, C + extra_channels) + rest)[:, :C]
    view.copy_(values)
    return view


def _parts(gen, B, Cs, C2, rest, extra_a=0, extra_b=0, sentinels=True):
    """(a, b, cat): the two fenced parts and their concatenation (an ordinary tensor)."""
    dev = _dev()
    a = torch.randn((B, Cs) + rest, generator=gen).to(dev)
    b = torch.randn((B, C2) + rest, generator=gen).to(dev)
    if sentinels:
        a[:, -1] = 1e30
        b[:, 0] = -1e30
    a, b = _fenced(a, extra_a), _fenced(b, extra_b)
    return a, b, torch.cat([a, b], 1).contiguous()


def _folded(gen, Cin, Cout, Cs, kshape, kind, act):
    """A folded layer with zero weights on the two channels at the seam (they carry the sentinels)."""
    from temporalstereo_amd.aggregation import native as N
    w = torch.randn((Cout, Cin) + kshape, generator=gen) / (Cin * kshape[1] * kshape[2]) ** 0.5
    w[:, Cs - 1] = 0.0
    w[:, Cs] = 0.0
    return N.Folded(w.to(_dev()), torch.randn(Cout, generator=gen).to(_dev()), None, act, False, kind)


def _same(new, old, what):
    torch.cuda.synchronize()
    assert bool(torch.isfinite(old).all()), (what, "the plain entry's result is not finite")
    assert torch.equal(new, old), (what, float((new - old).abs().max()))


# ------------------------------------------------------------------------------------------- ts_conv3d_hw_split_fwd (f32 MFMA kernel)
@pytest.mark.parametrize("B,Cout,dil", [(1, 8, 1), (1, 16, 1), (2, 8, 1), (2, 16, 1), (1, 8, 2)],
                         ids=lambda v: str(v))
def test_conv_hw_split_equals_the_concatenation(B, Cout, dil):
    """Cin 64 = 32 | 32 on 9 x 37 (ragged tile edges, W % 4 != 0: the f32 kernel): the row-paired Cout <= 8 form and the plain one,
    batch 2 with a different batch stride for each base, dilation 2."""
    from temporalstereo_amd.aggregation import native as N
    gen = torch.Generator().manual_seed(100 * B + 10 * Cout + dil)
    a, b, cat = _parts(gen, B, 32, 32, (1, 9, 37), extra_a=3 if B > 1 else 0, extra_b=1 if B > 1 else 0)
    assert B == 1 or a.stride(0) != b.stride(0)
    f = _folded(gen, 64, Cout, 32, (1, 3, 3), "hw", N.ACT_SILU)
    _same(N.conv_hw(N.Split(a, b), f, 1, dil), N.conv_hw(cat, f, 1, dil), ("conv_hw", B, Cout, dil))


def test_conv_hw_split_with_an_addend():
    from temporalstereo_amd.aggregation import native as N
    gen = torch.Generator().manual_seed(7)
    a, b, cat = _parts(gen, 2, 32, 32, (3, 9, 37), extra_a=2)
    f = _folded(gen, 64, 16, 32, (1, 3, 3), "hw", N.ACT_SILU)
    addend = torch.randn(2, 16, 1, 9, 37, generator=gen).to(_dev())
    _same(N.conv_hw(N.Split(a, b), f, addend=addend), N.conv_hw(cat, f, addend=addend), "conv_hw with an addend")


# ------------------------------------------------------------------------------------------- ts_conv3d_d_split_fwd
@pytest.mark.parametrize("B", [1, 2])
def test_conv_d_k1_split_equals_the_concatenation(B):
    """The Q pre-contraction's form: k = 1, Cin 64 = 32 | 32 -> 72 on 9 x 37."""
    from temporalstereo_amd.aggregation import native as N
    gen = torch.Generator().manual_seed(20 + B)
    a, b, cat = _parts(gen, B, 32, 32, (1, 9, 37), extra_b=2 if B > 1 else 0)
    f = _folded(gen, 64, 72, 32, (1, 1, 1), "d", N.ACT_NONE)
    _same(N.conv_d(N.Split(a, b), f, 1), N.conv_d(cat, f, 1), ("conv_d k = 1", B))


def test_conv_d_k3_split_equals_the_concatenation():
    from temporalstereo_amd.aggregation import native as N
    gen = torch.Generator().manual_seed(23)
    a, b, cat = _parts(gen, 1, 32, 32, (4, 9, 37))
    f = _folded(gen, 64, 16, 32, (3, 1, 1), "d", N.ACT_SILU)
    _same(N.conv_d(N.Split(a, b), f, 3, 1, 1, 1), N.conv_d(cat, f, 3, 1, 1, 1), "conv_d k = 3")


# ------------------------------------------------------------------------------------------- ts_conv3d_hw_x6_split_fwd (both kernels)
X6_CASES = [(1, 64, 32, 9, 36), (1, 64, 32, 17, 64), (1, 96, 64, 9, 36), (2, 96, 64, 17, 64)]       # B, Cin, Csplit, H, W; Cout 32


def _x6_cases():
    """Every x6 case through whichever x6 kernel this process dispatches to (ig_conv_x6_kernel on these grids unless TS_X6P_MIN_WGS
    forces the ping-pong form); returns how many were compared."""
    from temporalstereo_amd import _lib
    from temporalstereo_amd.aggregation import native as N
    N._X6_MIN_GRID = 1                  # small grids stay on the f32 kernel otherwise (tests/test_conv_x6_gpu.py does the same)
    n = 0
    for B, Cin, Cs, H, W in X6_CASES:
        assert _lib.lib().ts_conv3d_hw_x6_supported(Cin, 32, W, 1, 1, 0) == 1
        gen = torch.Generator().manual_seed(Cin + H)
        a, b, cat = _parts(gen, B, Cs, Cin - Cs, (1, H, W), extra_a=1 if B > 1 else 0, extra_b=2 if B > 1 else 0)
        for act in (N.ACT_SILU, N.ACT_NONE):
            f = _folded(gen, Cin, 32, Cs, (1, 3, 3), "hw", act)
            _same(N.conv_hw(N.Split(a, b), f), N.conv_hw(cat, f), ("x6", B, Cin, Cs, H, W, act))
            n += 1
    return n


def test_x6_split_equals_the_concatenation():
    """Cin 64 = 32 | 32 and 96 = 64 | 32 -> 32 on 9 x 36 and 17 x 64, ig_conv_x6_kernel."""
    from temporalstereo_amd.aggregation import native as N
    keep = N._X6_MIN_GRID
    try:
        assert _x6_cases() == 2 * len(X6_CASES)
    finally:
        N._X6_MIN_GRID = keep


@pytest.mark.parametrize("rows", ["8", "4"])
def test_x6_ping_pong_split_equals_the_concatenation(rows):
    """The same cases through ig_conv_x6p_kernel.  Its switches are read once per process, so -- as tests/test_conv_x6_gpu.py does --
    a child process runs them with the form forced on every grid (TS_X6P_MIN_WGS=1) and the half-tile height pinned."""
    env = dict(os.environ, TS_X6P_MIN_WGS="1", TS_X6P_HR=rows)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-x6"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and ("x6 split ok %d" % (2 * len(X6_CASES))) in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


def test_x6_on_a_width_it_does_not_take_is_refused_by_both_entries():
    """9 x 37: rows are staged as aligned quads, W % 4 != 0 is outside the x6 kernels -- the split entry refuses it exactly as the
    plain one does, and nothing is launched (conv_hw sends such a layer to the f32 kernel: the 9 x 37 cases above)."""
    from temporalstereo_amd import _lib
    from temporalstereo_amd.aggregation import native as N
    L = _lib.lib()
    gen = torch.Generator().manual_seed(3)
    a, b, cat = _parts(gen, 1, 32, 32, (1, 9, 37))
    f = _folded(gen, 64, 32, 32, (1, 3, 3), "hw", N.ACT_NONE)
    w6 = torch.zeros(int(L.ts_conv3d_hw_x6_weight_bytes(64, 32)), device=_dev(), dtype=torch.uint8)
    out = torch.full((1, 32, 1, 9, 37), NAN, device=_dev())
    plane = 9 * 37
    rc_old = L.ts_conv3d_hw_x6_fwd(_lib.ptr(cat), _lib.ptr(w6), _lib.ptr(f.scale), _lib.ptr(f.shift), _lib.ptr(out), 1, 64, 32, 1, 9, 37,
                                   1, 0, 0.0, 64 * plane, plane, 32 * plane, plane, None, 0, None, 0, N._stream())
    rc_new = L.ts_conv3d_hw_x6_split_fwd(_lib.ptr(a), _lib.ptr(b), _lib.ptr(w6), _lib.ptr(f.scale), _lib.ptr(f.shift), _lib.ptr(out), 1, 64,
                                         32, 32, 1, 9, 37, 1, 0, 0.0, a.stride(0), plane, b.stride(0), plane, 32 * plane, plane, None, 0,
                                         None, 0, N._stream())
    torch.cuda.synchronize()
    assert rc_old == UNSUPPORTED and rc_new == UNSUPPORTED
    assert L.ts_conv3d_hw_x6_split_supported(64, 32, 32, 37, 1) == 0
    assert bool(torch.isnan(out).all())


# ------------------------------------------------------------------------------------------- ts_block_cost_sampled_corr_split_fwd
@pytest.mark.parametrize("H,W,D", [(8, 40, 5), (9, 38, 5)], ids=lambda v: str(v))
@pytest.mark.parametrize("B", [1, 2])
def test_corr_blocks_split_equals_the_concatenation(B, H, W, D):
    """C 64 = 32 | 32, scales 3: block_cost_corr_rows (aligned rows) and the ragged np = 3 geometry (9, 38, 5), which runs
    block_cost_fast; left and right both split, every base with a batch stride of its own."""
    import temporalstereo_amd.functional as TF
    gen = torch.Generator().manual_seed(H * W + B)
    ex = (1, 2, 3, 5) if B > 1 else (0, 0, 0, 0)
    la, lb, lcat = _parts(gen, B, 32, 32, (H, W), extra_a=ex[0], extra_b=ex[1], sentinels=False)
    ra, rb, rcat = _parts(gen, B, 32, 32, (H, W), extra_a=ex[2], extra_b=ex[3], sentinels=False)
    disp = (torch.rand(B, D, H, W, generator=gen) * 14.0 - 2.0).to(_dev())
    _same(TF.block_cost_corr(TF.Split(la, lb), TF.Split(ra, rb), disp, 3), TF.block_cost_corr(lcat, rcat, disp, 3), ("corr", B, H, W, D))


# ------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("Cs", [20, 0, 64])
def test_seams_off_a_chunk_boundary_are_refused_without_a_launch(Cs):
    """Csplit = 20 (inside a chunk), 0 and Cin (no second / no first part): TS_ERR_UNSUPPORTED from every split entry, the
    *_split_supported queries say so beforehand, and the output is untouched."""
    from temporalstereo_amd import _lib
    from temporalstereo_amd.aggregation import native as N
    L = _lib.lib()
    dev = _dev()
    H, W, plane = 8, 40, 320
    x = torch.zeros(1, 64, 1, H, W, device=dev)
    w = torch.zeros(64 * 9 * 32, device=dev)
    sc = torch.ones(128, device=dev)
    out = torch.full((1, 32, 5, H, W), NAN, device=dev)
    ws = torch.zeros(1 << 20, device=dev, dtype=torch.uint8)
    w6 = torch.zeros(int(L.ts_conv3d_hw_x6_weight_bytes(64, 32)), device=dev, dtype=torch.uint8)
    p = _lib.ptr
    st = N._stream()
    assert L.ts_conv3d_hw_split_supported(1, 64, Cs, 32, 1, H, W, 1, 1, 0) == 0
    assert L.ts_conv3d_d_split_supported(64, Cs) == 0
    assert L.ts_conv3d_hw_x6_split_supported(64, Cs, 32, W, 1) == 0
    assert L.ts_block_cost_corr_split_supported(64, Cs) == 0
    rcs = [
        L.ts_conv3d_hw_split_fwd(p(x), p(x), p(w), p(sc), p(sc), p(out), 1, 64, Cs, 32, 1, H, W, 1, 1, 0, 0, 0.0, 64 * plane, plane,
                                 64 * plane, plane, 32 * 5 * plane, 5 * plane, None, 0, p(ws), ws.numel(), st),
        L.ts_conv3d_d_split_fwd(p(x), p(x), p(w), p(sc), p(sc), p(out), 1, 64, Cs, 32, 1, H, W, 1, 1, 1, 0, 0, 0, 0.0, 64 * plane, plane,
                                64 * plane, plane, 32 * 5 * plane, 5 * plane, st),
        L.ts_conv3d_hw_x6_split_fwd(p(x), p(x), p(w6), p(sc), p(sc), p(out), 1, 64, Cs, 32, 1, H, W, 1, 0, 0.0, 64 * plane, plane,
                                    64 * plane, plane, 32 * 5 * plane, 5 * plane, None, 0, p(ws), ws.numel(), st),
        L.ts_block_cost_sampled_corr_split_fwd(p(x), p(x), p(x), p(x), p(x), p(out), p(ws), 1, 64, Cs, H, W, 5, 3, 64 * plane,
                                               64 * plane, 64 * plane, 64 * plane, st),
    ]
    torch.cuda.synchronize()
    assert rcs == [UNSUPPORTED] * 4, rcs
    assert bool(torch.isnan(out).all())


# ------------------------------------------------------------------------------------------- the engine, end to end
def _tensors(out):
    """Every tensor an engine call returns, in a fixed order."""
    disps, costs, samples, offs, ranges, info = out
    ts = list(disps) + list(costs) + list(samples) + list(offs)
    for r in ranges:
        ts += [r['low'], r['high']]
    ts.append(info['prev_disp'])
    ts += [info['cost_memory']['disp_sample'], info['cost_memory']['cost_volume']]
    return [t.clone() for t in ts]


@pytest.mark.parametrize("B", [1, 2])
def test_engine_outputs_do_not_depend_on_split_input(B, monkeypatch):
    """96 x 160, a 32-channel 1/4 level (so that [feature | spx4] is 64 = 32 | 32): plain (eager) and as a recorded plan with three
    passes in flight, SPLIT_INPUT on and off -- every returned tensor bit-identical, the plan shorter by exactly the two feature
    copies and free of ts_copy_rows_fwd."""
    import bench
    import synth
    import temporalstereo_amd as ts
    from temporalstereo_amd.aggregation import native as N
    from temporalstereo_amd.aggregation.engine import InferenceEngine
    dev = _dev()
    seed = synth.SEED0 + 31
    net = ts.TEMPORALSTEREO(coarse=ts.CoarseAggregation(32, 8, 4), fine=ts.FineAggregation(16, 8, 5), precise=ts.PreciseAggregation(32, 8, 5))
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict({k: torch.from_numpy(v) for k, v in synth.state_values(shapes, seed).items()}, strict=True)
    net = net.to(dev)
    H, W = 96, 160
    lf, rf = synth.feature_pyramid(seed, B, H, W, chans=(32, 16, 32))
    il, ir = synth.images(seed, B, H, W)
    frame = ([torch.from_numpy(x).to(dev) for x in lf], [torch.from_numpy(x).to(dev) for x in rf],
             torch.from_numpy(il).to(dev), torch.from_numpy(ir).to(dev))
    bench.calibrate_batchnorm(net, frame)
    got, plans = {}, {}
    for on in (True, False):
        monkeypatch.setattr(N, "SPLIT_INPUT", on)
        eager = InferenceEngine(net, backend="native", replay="eager")
        got[on, "eager"] = _tensors(eager(*frame, {}))
        eng = InferenceEngine(net, backend="native", replay="plan", inputs="bind", pipeline=3)
        for _ in range(3):
            out = eng(*frame, {})
        torch.cuda.synchronize()
        got[on, "plan"] = _tensors(out)
        recs = [c.recorder for c in eng._graphs.values()]
        assert len(recs) == 3
        plans[on] = recs
    for kind in ("eager", "plan"):
        assert len(got[True, kind]) == len(got[False, kind]) > 10
        for i, (a, b) in enumerate(zip(got[True, kind], got[False, kind])):
            assert bool(torch.isfinite(b).all()) and torch.equal(a, b), (kind, i, float((a - b).abs().max()))
    for rec_on, rec_off in zip(plans[True], plans[False]):
        names_on, names_off = [n for n, _ in rec_on.log], [n for n, _ in rec_off.log]
        assert names_off.count("ts_copy_rows_fwd") == 2 and "ts_copy_rows_fwd" not in names_on
        assert len(rec_on) == len(rec_off) - 2 == len(names_on)
        assert "ts_conv3d_hw_split_fwd" in names_on and "ts_conv3d_d_split_fwd" in names_on and \
            "ts_block_cost_sampled_corr_split_fwd" in names_on


if __name__ == "__main__":
    if "--child-x6" in sys.argv:
        print("x6 split ok %d" % _x6_cases())
