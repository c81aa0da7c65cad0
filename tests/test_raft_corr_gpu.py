"""CorrBlock on the device (temporalstereo_amd.CorrBlock / raft_corr_pyramid / raft_corr_lookup; csrc/raft_corr.hip) against the
reference's own runs recorded in tests/golden/raft_corr_*.npz (tools/gen_golden.py --only-raft) and against tests/raft_ref.py in fp64
on the CPU, which tests/test_raft_corr_cpu.py pins to the same fixtures.

Bars, none taken from the code under test:
  pyramid, output   |hip - fp64 expectation| <= max(4 x dev32_64, (C + 4) 2^-24 A).  dev32_64 = max |fp32 run - fp64 run| of the
                    reference (fixture) or of raft_ref on the CPU (shapes d, f).  A = max sum_c |fmap1| |fmap2| / sqrt(C) over the row
                    pairs, in fp64: the bound of a C-term fp32 dot product summed in any order, plus four roundings for the scale,
                    the pooling, the interpolation and the level weight.  The factor 4: a second, equally rounded evaluation may land
                    twice as far from fp64 as the first; 4 leaves a factor of two.  Each case prints error / bar; with
                    TS_RAFT_PARITY_FILE set the line is appended to that file (that is how profiles/raft_corr_parity.txt is made).
  exact answers     where every fp32 step is exact (W - 1 a power of two, constant pyramid, dyadic disparities) the output is the
                    fp64 expectation bit for bit: 0, the level weights 1 - 2^-(i+1) and their halves at the row's ends.  A window
                    entirely outside the row: exact zeros, zero grad_disp.
  gradients         relative L2 against fp64 autograd of raft_ref <= max(4 x the fp32 torch run's own relative L2, 1e-6); against the
                    stored gradients of the reference's fp32 run: that bar plus the stored run's own relative L2 (triangle inequality).
  backward          bit-equal over two runs;  forward  bit-equal when replayed from a captured graph.
"""
import functools

import numpy as np
import pytest
import torch

import raft_ref as R
from compare import Parity, gpu, rel_l2, same_bits
import temporalstereo_amd as ts

pytestmark = pytest.mark.gpu

report = Parity("TS_RAFT_PARITY_FILE").report
#        tag  B  C   H   W   L  r
SHAPES = {"a": (2, 6, 3, 37, 4, 4),        # batch stride; C no multiple of the MFMA K step; W ragged against 16; 37 -> 18 -> 9 -> 4
          "b": (1, 5, 2, 66, 4, 4),        # two columns past one 64-pixel strip; 66 -> 33 -> 16 -> 8
          "c": (1, 40, 1, 8, 4, 1),        # one row; C past one 32-channel chunk; last level of width 1; smallest window
          "e": (1, 32, 4, 64, 3, 2),       # fully aligned; L != 4; r != 4
          "d": (1, 16, 33, 130, 4, 4),     # more rows than one workgroup covers; more than one tile along x and x' (no fixture)
          "f": (1, 3, 2, 9, 1, 4)}         # single level; window wider than the row (no fixture)
FIXTURES = ("a", "b", "c", "e")
TAGS = tuple(SHAPES)


def off_the_kinks(disp, rng, W, L, r):
    """the generator's rule for a shape without a fixture: single disparities drawn again until, in fp64, no position of any level or
    tap lies within 1e-3 of an integer and the fp32 and fp64 floors agree"""
    def bad_pixels(d):
        bad = torch.zeros(d.shape, dtype=torch.bool)
        for i in range(L):
            x64, x32 = R.positions(d.double(), i, r, W >> i), R.positions(d, i, r, W >> i)
            b = ((x64 - torch.round(x64)).abs() < 1e-3) | (torch.floor(x64) != torch.floor(x32.double()))
            bad |= b.any(dim=-1).unsqueeze(1)
        return bad
    for _ in range(200):
        bad = bad_pixels(disp)
        n = int(bad.sum())
        if n == 0:
            return disp
        disp[bad] = torch.from_numpy(rng.uniform(-0.2, 0.7, size=n) * W).float()
    raise AssertionError("no disparity map off the kinks found")


@functools.lru_cache(maxsize=None)
def case(tag):
    """inputs (CPU, fp32), the fp64 expectation, the fp32 runs' deviations from it and the gradients in fp64, computed once"""
    B, C, H, W, L, r = SHAPES[tag]
    c = {}
    if tag in FIXTURES:
        g = R.load_fixture(tag)
        f1, f2, disp, cot = (torch.from_numpy(g[k]) for k in ("fmap1", "fmap2", "disp", "cot"))
        c["stored"] = {k: torch.from_numpy(g["grad_" + k]) for k in ("fmap1", "fmap2", "disp")}
        c["stored_rel"] = {k: float(g["rel_grad_" + k]) for k in ("fmap1", "fmap2", "disp")}
    else:
        rng = np.random.default_rng(40260 + ord(tag))
        f = lambda a: torch.from_numpy(a).float()
        f1, f2 = f(rng.normal(size=(B, C, H, W))), f(rng.normal(size=(B, C, H, W)))
        disp = off_the_kinks(f(rng.uniform(-0.2, 0.7, size=(B, 1, H, W)) * W), rng, W, L, r)
        cot = f(rng.integers(-8, 9, size=(B, L * (2 * r + 1), H, W)) / 8.0)
    assert tuple(f1.shape) == (B, C, H, W) and tuple(disp.shape) == (B, 1, H, W)

    def run(dt):
        a, b_, d = (t.detach().clone().to(dt).requires_grad_(True) for t in (f1, f2, disp))
        levels = R.corr_pyramid(a, b_, L)
        out = R.lookup(levels, d, r)
        out.backward(cot.to(dt))
        return [p.detach() for p in levels], out.detach(), {"fmap1": a.grad, "fmap2": b_.grad, "disp": d.grad}
    lv64, o64, g64 = run(torch.float64)
    lv32, o32, g32 = run(torch.float32)
    if tag in FIXTURES:
        dev_pyr, dev_out = [float(g["dev_pyr_%d" % i]) for i in range(L)], float(g["dev_out"])
    else:
        dev_pyr, dev_out = [float((a.double() - b_).abs().max()) for a, b_ in zip(lv32, lv64)], float((o32.double() - o64).abs().max())
    c.update(fmap1=f1, fmap2=f2, disp=disp, cot=cot, levels64=lv64, out64=o64, grads64=g64, dev_pyr=dev_pyr, dev_out=dev_out,
             rel32={k: rel_l2(g32[k], g64[k]) for k in g64}, floor=(C + 4) * 2.0 ** -24 * R.dot_bound(f1, f2))
    # the lookup alone, differentiated with respect to a free pyramid (fp32 values of the fp64 levels, so that both runs start equal)
    def run_lookup(dt):
        leaves = [p.float().to(dt).requires_grad_(True) for p in lv64]
        R.lookup(leaves, disp.to(dt), r).backward(cot.to(dt))
        return [p.grad for p in leaves]
    gp64, gp32 = run_lookup(torch.float64), run_lookup(torch.float32)
    c.update(gpyr64=gp64, gpyr_rel32=[rel_l2(a, b_) for a, b_ in zip(gp32, gp64)])
    return c


def flat_pyramid(levels, dtype=torch.float32):
    """the levels [B,H,W,W_i] as the one buffer of the library"""
    return torch.cat([p.reshape(-1) for p in levels]).to(dtype)


@pytest.mark.parametrize("tag", TAGS)
def test_pyramid_forward(tag):
    B, C, H, W, L, r = SHAPES[tag]
    c = case(tag)
    pyr = ts.raft_corr_pyramid(gpu(c["fmap1"]), gpu(c["fmap2"]), L)
    assert pyr.dtype == torch.float32 and pyr.dim() == 1 and pyr.numel() == B * H * W * sum(W >> i for i in range(L))
    views = ts.functional.raft_corr_level_views(pyr, B, H, W, L)
    worst = 0.0
    for i in range(L):
        assert tuple(views[i].shape) == (B * H * W, 1, 1, W >> i)
        err = float((views[i].cpu().double().reshape(B, H, W, W >> i) - c["levels64"][i]).abs().max())
        bar = max(4 * c["dev_pyr"][i], c["floor"])
        report("raft_corr parity pyramid  %s level %d  err %.3e  dev32_64 %.3e  bar %.3e  err/bar %.3f" % (tag, i, err, c["dev_pyr"][i], bar, err / bar))
        worst = max(worst, err / bar)
    assert worst <= 1.0


@pytest.mark.parametrize("tag", TAGS)
def test_lookup_forward(tag):
    B, C, H, W, L, r = SHAPES[tag]
    c = case(tag)
    with torch.no_grad():
        out = ts.CorrBlock(gpu(c["fmap1"]), gpu(c["fmap2"]), num_levels=L, radius=r)(gpu(c["disp"]))
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (B, L * (2 * r + 1), H, W)
    err = float((out.cpu().double() - c["out64"]).abs().max())
    bar = max(4 * c["dev_out"], c["floor"])
    report("raft_corr parity output   %s          err %.3e  dev32_64 %.3e  bar %.3e  err/bar %.3f" % (tag, err, c["dev_out"], bar, err / bar))
    assert err <= bar
    zeros = c["out64"] == 0
    assert bool(zeros.any()) and bool((out.cpu()[zeros] == 0).all())          # windows outside the row: exact zeros


def test_exact_answers_one_hot_rows():
    """as test_exact_answers, with rows that are one-hot along x': fmap1 = fmap2 = 1 in channel x mod 16 of 16, so P_0[x][x'] is 1/4
    where x' == x (mod 16) and 0 elsewhere, every level a dyadic spike, and reading a wrong cell or another pixel's row shows"""
    B, H, W, L, r = 1, 3, 17, 3, 2
    f = torch.zeros(B, 16, H, W)
    for x in range(W):
        f[:, x % 16, :, x] = 1.0
    rng = np.random.default_rng(6)
    disp = torch.from_numpy(rng.integers(-16, 49, size=(B, 1, H, W)) / 4.0).float()
    blk = ts.CorrBlock(gpu(f), gpu(f), num_levels=L, radius=r)
    lv64 = R.corr_pyramid(f.double(), f.double(), L)
    for i in range(L):
        assert torch.equal(blk.corr_pyramid[i].cpu().double().reshape(lv64[i].shape), lv64[i])
    assert float(lv64[0][0, 0, 5, 5]) == 0.25 and float(lv64[0][0, 0, 5, 6]) == 0.0 and float(lv64[1][0, 0, 5, 2]) == 0.125
    out = blk(gpu(disp)).cpu()
    exp64 = R.lookup(lv64, disp.double(), r)
    assert torch.equal(out.double(), exp64)
    assert 0.02 < float((exp64 != 0).double().mean()) < 0.9


@pytest.mark.parametrize("hot", ("ones_C1", "one_hot_C4"))
def test_exact_answers(hot):
    """W - 1 = 16 and disparities that are multiples of 1/4: every step of the fp32 sequence is exact, the pyramid is constant (1, or
    1/2 from one hot channel of four), so the output IS the fp64 expectation: 0 outside, the level weight times the constant at
    integer and half-integer positions inside, half of it half a cell off either end"""
    B, H, W, L, r = 1, 3, 17, 3, 2
    if hot == "ones_C1":
        f = torch.ones(B, 1, H, W)
        const = 1.0
    else:
        f = torch.zeros(B, 4, H, W)
        f[:, 2] = 1.0
        const = 0.5
    rng = np.random.default_rng(5)
    disp = torch.from_numpy(rng.integers(-16, 49, size=(B, 1, H, W)) / 4.0).float()
    disp[0, 0, 0, :4] = torch.tensor([0.0, 1.0, -6.0, 40.0])
    blk = ts.CorrBlock(gpu(f), gpu(f), num_levels=L, radius=r)
    for i in range(L):
        assert bool((blk.corr_pyramid[i] == const).all())
    out = blk(gpu(disp)).cpu()
    exp64 = R.corr_block(f.double(), f.double(), disp.double(), L, r)
    assert same_bits(out, exp64.float()) and torch.equal(out.double(), exp64)
    K, ends_seen = 2 * r + 1, False
    for i in range(L):
        Wi, wy = W >> i, 1.0 - 0.5 ** (i + 1)
        xp = R.positions(disp.double(), i, r, Wi).permute(0, 3, 1, 2)
        o = out[:, i * K:(i + 1) * K].double()
        inside = (xp >= 0) & (xp <= Wi - 1) & (xp * 2 == torch.round(xp * 2))
        ends = (xp == -0.5) | (xp == Wi - 0.5)
        outside = (xp <= -1) | (xp >= Wi)
        assert bool((o[inside] == wy * const).all()) and bool((o[ends] == wy * const / 2).all()) and bool((o[outside] == 0).all())
        ends_seen = ends_seen or bool(ends.any())
        assert bool(inside.any()) and bool(outside.any())
    assert ends_seen


def test_window_entirely_outside():
    B, C, H, W, L, r = SHAPES["a"]
    c = case("a")
    # level i sees x - disp divided by 2^i AND scaled by W_i / (W - 1), about (x - disp) / 4^i cells: 20 W puts level 3 outside too
    for shift in (20.0 * W, -20.0 * W):
        f1, f2 = gpu(c["fmap1"]).requires_grad_(True), gpu(c["fmap2"]).requires_grad_(True)
        disp = gpu(torch.full((B, 1, H, W), shift)).requires_grad_(True)
        out = ts.CorrBlock(f1, f2, num_levels=L, radius=r)(disp)
        assert bool((out == 0).all())
        out.backward(gpu(c["cot"]))
        assert bool((disp.grad == 0).all()) and bool((f1.grad == 0).all()) and bool((f2.grad == 0).all())


def _grads(tag, composed):
    B, C, H, W, L, r = SHAPES[tag]
    c = case(tag)
    f1, f2, d = (gpu(c[k]).requires_grad_(True) for k in ("fmap1", "fmap2", "disp"))
    if composed == "block":
        out = ts.CorrBlock(f1, f2, num_levels=L, radius=r)(d)
    else:
        out = ts.raft_corr_lookup(ts.raft_corr_pyramid(f1, f2, L), d, r)
    out.backward(gpu(c["cot"]))
    return {"fmap1": f1.grad, "fmap2": f2.grad, "disp": d.grad}


@pytest.mark.parametrize("composed", ("block", "functional"))
@pytest.mark.parametrize("tag", TAGS)
def test_gradients_build_and_lookup(tag, composed):
    c = case(tag)
    got = _grads(tag, composed)
    worst = 0.0
    for k in ("fmap1", "fmap2", "disp"):
        rel, bar = rel_l2(got[k].cpu(), c["grads64"][k]), max(4 * c["rel32"][k], 1e-6)
        line = "raft_corr parity grad %-5s %s %-10s rel %.3e  fp32 torch %.3e  bar %.3e  rel/bar %.3f" % (k, tag, composed, rel, c["rel32"][k], bar, rel / bar)
        worst = max(worst, rel / bar)
        if tag in FIXTURES:
            rs, bs = rel_l2(got[k].cpu(), c["stored"][k]), bar + c["stored_rel"][k]
            line += "  | vs the reference's fp32 run %.3e  bar %.3e" % (rs, bs)
            worst = max(worst, rs / bs)
        report(line)
    assert worst <= 1.0


@pytest.mark.parametrize("tag", TAGS)
def test_gradient_of_the_lookup_alone(tag):
    B, C, H, W, L, r = SHAPES[tag]
    c = case(tag)
    pyr = gpu(flat_pyramid(c["levels64"])).requires_grad_(True)
    d = gpu(c["disp"]).requires_grad_(True)
    out = ts.raft_corr_lookup(pyr, d, r)
    exp = R.lookup([p.float().double() for p in c["levels64"]], c["disp"].double(), r)
    assert float((out.detach().cpu().double() - exp).abs().max()) <= max(4 * c["dev_out"], c["floor"])
    out.backward(gpu(c["cot"]))
    got = ts.functional.raft_corr_level_views(pyr.grad, B, H, W, L)
    worst = 0.0
    for i in range(L):
        rel, bar = rel_l2(got[i].cpu().reshape(c["gpyr64"][i].shape), c["gpyr64"][i]), max(4 * c["gpyr_rel32"][i], 1e-6)
        report("raft_corr parity grad level %d %s lookup    rel %.3e  fp32 torch %.3e  bar %.3e  rel/bar %.3f" % (i, tag, rel, c["gpyr_rel32"][i], bar, rel / bar))
        worst = max(worst, rel / bar)
    assert worst <= 1.0


def test_backward_is_bit_reproducible():
    a, b = _grads("d", "block"), _grads("d", "block")
    for k in a:
        assert same_bits(a[k], b[k]), k
    a, b = _grads("d", "functional"), _grads("d", "functional")
    for k in a:
        assert same_bits(a[k], b[k]), k


def test_forward_replays_from_a_captured_graph():
    B, C, H, W, L, r = SHAPES["b"]
    c = case("b")
    f1, f2, d = gpu(c["fmap1"]), gpu(c["fmap2"]), gpu(c["disp"])
    with torch.no_grad():
        eager = ts.CorrBlock(f1, f2, num_levels=L, radius=r)(d)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            ts.CorrBlock(f1, f2, num_levels=L, radius=r)(d)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = ts.CorrBlock(f1, f2, num_levels=L, radius=r)(d)
        captured.zero_()
        graph.replay()
        torch.cuda.synchronize()
    assert same_bits(captured, eager)


def test_api():
    B, C, H, W, L, r = SHAPES["a"]
    c = case("a")
    f1, f2, d = gpu(c["fmap1"]), gpu(c["fmap2"]), gpu(c["disp"])
    blk = ts.CorrBlock(f1, f2)
    assert (blk.num_levels, blk.radius) == (4, 4) and len(blk.corr_pyramid) == 4
    for i in range(4):
        assert tuple(blk.corr_pyramid[i].shape) == (B * H * W, 1, 1, W >> i)
    out = blk(d)
    assert same_bits(out, ts.raft_corr_lookup(ts.raft_corr_pyramid(f1, f2, 4), d, 4))
    assert same_bits(ts.CorrBlock(f1, f2, num_levels=2, radius=1)(d), ts.raft_corr_lookup(ts.raft_corr_pyramid(f1, f2, 2), d, 1))
    assert tuple(ts.CorrBlock(f1, f2, num_levels=1, radius=0)(d).shape) == (B, 1, H, W)


def test_refusals():
    B, C, H, W, L, r = SHAPES["a"]
    c = case("a")
    f1, f2, d = gpu(c["fmap1"]), gpu(c["fmap2"]), gpu(c["disp"])
    with pytest.raises(TypeError, match="fp32"):
        ts.CorrBlock(f1.double(), f2.double())
    with pytest.raises(TypeError, match="fp32"):
        ts.CorrBlock(f1, f2)(d.half())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ts.CorrBlock(f1.cpu(), f2.cpu())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ts.CorrBlock(f1, f2)(d.cpu())
    with pytest.raises(ValueError, match="differ in shape"):
        ts.CorrBlock(f1, f2[:, :, :, :W - 1])
    with pytest.raises(ValueError, match="does not match"):
        ts.CorrBlock(f1, f2)(d[:, :, :H - 1])
    with pytest.raises(ValueError, match="1 channel"):
        ts.CorrBlock(f1, f2)(torch.cat([d, d], dim=1))
    with pytest.raises(ValueError, match="W >= 2"):
        ts.CorrBlock(f1[..., :1], f2[..., :1], num_levels=1)
    with pytest.raises(ValueError, match="too narrow"):
        ts.CorrBlock(f1[..., :7], f2[..., :7], num_levels=4)
    assert tuple(ts.CorrBlock(f1[..., :8], f2[..., :8], num_levels=4).corr_pyramid[3].shape) == (B * H * 8, 1, 1, 1)
    with pytest.raises(ValueError, match="num_levels must be >= 1"):
        ts.CorrBlock(f1, f2, num_levels=0)
    with pytest.raises(ValueError, match="radius must be >= 0"):
        ts.CorrBlock(f1, f2, radius=-1)
    with pytest.raises(ValueError, match="radius must be >= 0"):
        ts.raft_corr_lookup(ts.raft_corr_pyramid(f1, f2, 2), d, -1)
    with pytest.raises(ValueError, match="no pyramid of width"):
        ts.raft_corr_lookup(ts.raft_corr_pyramid(f1, f2, 2)[:-B * H * W], d, 1)
