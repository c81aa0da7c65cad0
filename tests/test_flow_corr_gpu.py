"""FlowCorrBlock on the device (temporalstereo_amd.FlowCorrBlock / flow_corr_pyramid / flow_corr_lookup; csrc/flow_corr.hip) against
the reference's own runs recorded in tests/golden/flow_corr_*.npz (tools/gen_golden.py --only-flow) and against
tests/flow_corr_ref.py in fp64 on the CPU, which tests/test_flow_corr_cpu.py pins to the same fixtures.

Bars, none taken from the code under test:
  pyramid, output   |hip - fp64 expectation| <= max(4 x dev32_64, (2C + 8) 2^-24 A).  dev32_64 = max |fp32 run - fp64 run| of the
                    reference (fixture) or of flow_corr_ref on the CPU (shapes b, d, f).  A = max over the pixel pairs of
                    (sum |f1_n||f1_m| + 2 sum |f1_n||f2_m| + sum |f2_n||f2_m|) / sqrt(C), in fp64: the bound of an fp32 dot product of
                    up to 2C terms summed in any order (three Gram matrices of C terms, or one contraction of f1 | f1 - f2 against
                    f1 - f2 | f2), plus eight roundings for the difference, the scale, the combine, the pooling and the
                    interpolation.  The factor 4 is argued in tests/test_raft_corr_gpu.py's docstring.  Each case prints error /
                    bar; with TS_FLOW_PARITY_FILE set the line is appended to that file (profiles/flow_corr_parity.txt is made so).
  exact answers     H = W = 5, L = 2, r = 1, even integer coordinates: W_i - 1 and H_i - 1 are 4 and 1, every fp32 step of the
                    position is exact and every bilinear weight is 0 or 1, so every output IS, bit for bit, the cell
                    (y_t / 2^i + b - r, x_t / 2^i + a - r) of the device's own pyramid, or 0 outside.  The cells of a row are
                    distinct (asserted), which pins the tap order and the channel order.  A window entirely outside the map: exact
                    zeros, zero grad_coords.
  gradients         relative L2 against fp64 autograd of flow_corr_ref <= max(4 x the fp32 torch run's own relative L2, 1e-6); against
                    the stored gradients of the reference's fp32 run: that bar plus the stored run's own relative L2 (triangle
                    inequality).
  backward          bit-equal over two runs;  forward  bit-equal when replayed from a captured graph.
"""
import functools

import numpy as np
import pytest
import torch

import flow_corr_ref as R
from compare import Parity, dev as _dev, gpu, rel_l2, same_bits
import temporalstereo_amd as ts

pytestmark = pytest.mark.gpu

report = Parity("TS_FLOW_PARITY_FILE").report
#        tag  B  C   H   W   L  r
SHAPES = {"a": (2, 6, 8, 11, 3, 2),        # batch stride; C no multiple of the MFMA step; ragged against every tile edge; 8x11 -> 4x5 -> 2x2, a dropped column
          "c": (1, 40, 4, 4, 2, 1),        # C past one staged chunk; last level 2x2, the smallest legal
          "e": (1, 32, 8, 16, 3, 3),       # fully aligned
          "b": (1, 5, 4, 70, 2, 1),        # image row longer than a 64-wide tile edge; N = 280 (no fixture)
          "d": (1, 16, 17, 33, 4, 4),      # the reference's defaults; several tiles along n and both patch directions; odd H, W at every level (no fixture)
          "f": (1, 3, 2, 3, 1, 4)}         # single level; window far wider than the map (no fixture)
FIXTURES = ("a", "c", "e")
TAGS = tuple(SHAPES)
GRADS = ("fmap1", "fmap2", "coords")


def pixel_grid(B, H, W):
    return ts.FlowCorrBlock.init_flow((B, 1, H, W), "cpu")[0].double()


def off_the_kinks(rng, B, H, W, L, r):
    """the generator's rule for a shape without a fixture: the pixel grid plus a flow uniform in +-0.25 (W, H), single pixels drawn again
    until, in fp64, no position of any level or tap lies within 1e-3 of an integer and the fp32 and fp64 floors agree"""
    grid = pixel_grid(B, H, W).permute(0, 2, 3, 1)                             # [B,H,W,2]
    span = torch.tensor([W, H], dtype=torch.float64)
    draw = lambda n: torch.from_numpy(rng.uniform(-0.25, 0.25, size=(n, 2))) * span
    coords = (grid + draw(B * H * W).view(B, H, W, 2)).float()

    def bad_pixels(c):
        c = c.permute(0, 3, 1, 2)
        bad = torch.zeros((B, H, W), dtype=torch.bool)
        for i in range(L):
            for a64, a32 in zip(R.positions(c.double(), i, r, H >> i, W >> i), R.positions(c, i, r, H >> i, W >> i)):
                bad |= (((a64 - torch.round(a64)).abs() < 1e-3) | (torch.floor(a64) != torch.floor(a32.double()))).any(dim=-1)
        return bad
    for _ in range(200):
        bad = bad_pixels(coords)
        n = int(bad.sum())
        if n == 0:
            return coords.permute(0, 3, 1, 2).contiguous()
        coords[bad] = (grid[bad] + draw(n)).float()
    raise AssertionError("no coordinates off the kinks found")


@functools.lru_cache(maxsize=None)
def case(tag):
    """inputs (CPU, fp32), the fp64 expectation, the fp32 runs' deviations from it and the gradients in fp64, computed once"""
    B, C, H, W, L, r = SHAPES[tag]
    c = {}
    if tag in FIXTURES:
        g = R.load_fixture(tag)
        f1, f2, coords, cot = (torch.from_numpy(g[k]) for k in ("fmap1", "fmap2", "coords", "cot"))
        c["stored"] = {k: torch.from_numpy(g["grad_" + k]) for k in GRADS}
        c["stored_rel"] = {k: float(g["rel_grad_" + k]) for k in GRADS}
    else:
        rng = np.random.default_rng(50260 + ord(tag))
        f = lambda a: torch.from_numpy(a).float()
        f1, f2 = f(rng.normal(size=(B, C, H, W))), f(rng.normal(size=(B, C, H, W)))
        coords = off_the_kinks(rng, B, H, W, L, r)
        cot = f(rng.integers(-8, 9, size=(B, L * (2 * r + 1) ** 2, H, W)) / 8.0)
    assert tuple(f1.shape) == (B, C, H, W) and tuple(coords.shape) == (B, 2, H, W)

    def run(dt):
        a, b_, d = (t.detach().clone().to(dt).requires_grad_(True) for t in (f1, f2, coords))
        levels = R.corr_pyramid(a, b_, L)
        out = R.lookup(levels, d, r)
        out.backward(cot.to(dt))
        return [p.detach() for p in levels], out.detach(), {"fmap1": a.grad, "fmap2": b_.grad, "coords": d.grad}
    lv64, o64, g64 = run(torch.float64)
    lv32, o32, g32 = run(torch.float32)
    if tag in FIXTURES:
        dev_pyr, dev_out = [float(g["dev_pyr_%d" % i]) for i in range(L)], float(g["dev_out"])
    else:
        dev_pyr, dev_out = [float((a.double() - b_).abs().max()) for a, b_ in zip(lv32, lv64)], float((o32.double() - o64).abs().max())
    c.update(fmap1=f1, fmap2=f2, coords=coords, cot=cot, levels64=lv64, out64=o64, grads64=g64, dev_pyr=dev_pyr, dev_out=dev_out,
             rel32={k: rel_l2(g32[k], g64[k]) for k in g64}, floor=(2 * C + 8) * 2.0 ** -24 * R.dot_bound(f1, f2))
    # the lookup alone, differentiated with respect to a free pyramid (fp32 values of the fp64 levels, so that both runs start equal)
    def run_lookup(dt):
        leaves = [p.float().to(dt).requires_grad_(True) for p in lv64]
        R.lookup(leaves, coords.to(dt), r).backward(cot.to(dt))
        return [p.grad for p in leaves]
    gp64, gp32 = run_lookup(torch.float64), run_lookup(torch.float32)
    c.update(gpyr64=gp64, gpyr_rel32=[rel_l2(a, b_) for a, b_ in zip(gp32, gp64)])
    return c


def flat_pyramid(levels, dtype=torch.float32):
    """the levels [B,N,H_i,W_i] as the one buffer of the library"""
    return torch.cat([p.reshape(-1) for p in levels]).to(dtype)


@pytest.mark.parametrize("tag", TAGS)
def test_pyramid_forward(tag):
    B, C, H, W, L, r = SHAPES[tag]
    c = case(tag)
    pyr = ts.flow_corr_pyramid(gpu(c["fmap1"]), gpu(c["fmap2"]), L)
    assert pyr.dtype == torch.float32 and pyr.dim() == 1 and pyr.numel() == B * H * W * sum((H >> i) * (W >> i) for i in range(L))
    views = ts.flow_corr_level_views(pyr, B, H, W, L)
    worst = 0.0
    for i in range(L):
        assert tuple(views[i].shape) == (B * H * W, 1, H >> i, W >> i)
        err = float((views[i].cpu().double().reshape(c["levels64"][i].shape) - c["levels64"][i]).abs().max())
        bar = max(4 * c["dev_pyr"][i], c["floor"])
        report("flow_corr parity pyramid  %s level %d  err %.3e  dev32_64 %.3e  bar %.3e  err/bar %.3f" % (tag, i, err, c["dev_pyr"][i], bar, err / bar))
        worst = max(worst, err / bar)
    assert worst <= 1.0


@pytest.mark.parametrize("tag", TAGS)
def test_lookup_forward(tag):
    B, C, H, W, L, r = SHAPES[tag]
    c = case(tag)
    with torch.no_grad():
        out = ts.FlowCorrBlock(gpu(c["fmap1"]), gpu(c["fmap2"]), num_levels=L, radius=r)(gpu(c["coords"]))
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (B, L * (2 * r + 1) ** 2, H, W)
    err = float((out.cpu().double() - c["out64"]).abs().max())
    bar = max(4 * c["dev_out"], c["floor"])
    report("flow_corr parity output   %s          err %.3e  dev32_64 %.3e  bar %.3e  err/bar %.3f" % (tag, err, c["dev_out"], bar, err / bar))
    assert err <= bar
    zeros = c["out64"] == 0
    assert bool(zeros.any()) and bool((out.cpu()[zeros] == 0).all())          # taps outside the map: exact zeros


def test_exact_answers():
    """H = W = 5, L = 2, r = 1 and even integer coordinates: every output is a cell of the device's own pyramid, or 0 (see the bars)"""
    B, C, H, W, L, r = 2, 7, 5, 5, 2, 1
    K = 2 * r + 1
    rng = np.random.default_rng(7)
    f1, f2 = (torch.from_numpy(rng.normal(size=(B, C, H, W))).float() for _ in range(2))
    coords = torch.from_numpy(rng.integers(-1, 4, size=(B, 2, H, W)) * 2.0).float()          # -2 .. 6: some windows leave the map
    coords[0, :, 0, 0] = torch.tensor([0.0, 4.0])                                            # x != y: a transposed window would show
    blk = ts.FlowCorrBlock(gpu(f1), gpu(f2), num_levels=L, radius=r)
    out = blk(gpu(coords)).cpu()
    assert tuple(out.shape) == (B, L * K * K, H, W)
    expect = torch.zeros_like(out)
    inside = 0
    for i in range(L):
        Hi, Wi = H >> i, W >> i
        P = blk.corr_pyramid[i].cpu().reshape(B, H, W, Hi, Wi)
        rows = P.reshape(B * H * W, Hi * Wi)
        assert all(torch.unique(row).numel() == row.numel() for row in rows)                 # distinct cells in every row
        for a in range(K):
            for b in range(K):
                for bi in range(B):
                    for y in range(H):
                        for x in range(W):
                            cx, cy = int(coords[bi, 0, y, x]) // 2 ** i + a - r, int(coords[bi, 1, y, x]) // 2 ** i + b - r
                            if 0 <= cx < Wi and 0 <= cy < Hi:
                                expect[bi, i * K * K + a * K + b, y, x] = P[bi, y, x, cy, cx]
                                inside += 1
    assert same_bits(out, expect)
    assert 0.2 < inside / out.numel() < 0.9


def test_window_entirely_outside():
    B, C, H, W, L, r = SHAPES["a"]
    c = case("a")
    for shift in (1000.0, -1000.0):
        f1, f2 = gpu(c["fmap1"]).requires_grad_(True), gpu(c["fmap2"]).requires_grad_(True)
        coords = gpu(torch.full((B, 2, H, W), shift)).requires_grad_(True)
        out = ts.FlowCorrBlock(f1, f2, num_levels=L, radius=r)(coords)
        assert bool((out == 0).all())
        out.backward(gpu(c["cot"]))
        assert bool((coords.grad == 0).all()) and bool((f1.grad == 0).all()) and bool((f2.grad == 0).all())


def _grads(tag, composed):
    B, C, H, W, L, r = SHAPES[tag]
    c = case(tag)
    f1, f2, d = (gpu(c[k]).requires_grad_(True) for k in GRADS)
    if composed == "block":
        out = ts.FlowCorrBlock(f1, f2, num_levels=L, radius=r)(d)
    else:
        out = ts.flow_corr_lookup(ts.flow_corr_pyramid(f1, f2, L), d, r, size=(H, W))
    out.backward(gpu(c["cot"]))
    return {"fmap1": f1.grad, "fmap2": f2.grad, "coords": d.grad}


@pytest.mark.parametrize("composed", ("block", "functional"))
@pytest.mark.parametrize("tag", TAGS)
def test_gradients_build_and_lookup(tag, composed):
    c = case(tag)
    got = _grads(tag, composed)
    worst = 0.0
    for k in GRADS:
        rel, bar = rel_l2(got[k].cpu(), c["grads64"][k]), max(4 * c["rel32"][k], 1e-6)
        line = "flow_corr parity grad %-6s %s %-10s rel %.3e  fp32 torch %.3e  bar %.3e  rel/bar %.3f" % (k, tag, composed, rel, c["rel32"][k], bar, rel / bar)
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
    d = gpu(c["coords"]).requires_grad_(True)
    out = ts.flow_corr_lookup(pyr, d, r)
    exp = R.lookup([p.float().double() for p in c["levels64"]], c["coords"].double(), r)
    assert float((out.detach().cpu().double() - exp).abs().max()) <= max(4 * c["dev_out"], c["floor"])
    out.backward(gpu(c["cot"]))
    got = ts.flow_corr_level_views(pyr.grad, B, H, W, L)
    worst = 0.0
    for i in range(L):
        rel, bar = rel_l2(got[i].cpu().reshape(c["gpyr64"][i].shape), c["gpyr64"][i]), max(4 * c["gpyr_rel32"][i], 1e-6)
        report("flow_corr parity grad level %d %s lookup    rel %.3e  fp32 torch %.3e  bar %.3e  rel/bar %.3f" % (i, tag, rel, c["gpyr_rel32"][i], bar, rel / bar))
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
    f1, f2, d = gpu(c["fmap1"]), gpu(c["fmap2"]), gpu(c["coords"])
    with torch.no_grad():
        eager = ts.FlowCorrBlock(f1, f2, num_levels=L, radius=r)(d)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            ts.FlowCorrBlock(f1, f2, num_levels=L, radius=r)(d)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            captured = ts.FlowCorrBlock(f1, f2, num_levels=L, radius=r)(d)
        captured.zero_()
        graph.replay()
        torch.cuda.synchronize()
    assert same_bits(captured, eager)


def test_api():
    B, C, H, W, L, r = SHAPES["d"]
    c = case("d")
    f1, f2, d = gpu(c["fmap1"]), gpu(c["fmap2"]), gpu(c["coords"])
    blk = ts.FlowCorrBlock(f1, f2)
    assert (blk.num_levels, blk.radius) == (4, 4) and len(blk.corr_pyramid) == 4
    for i in range(4):
        assert tuple(blk.corr_pyramid[i].shape) == (B * H * W, 1, H >> i, W >> i)
    out = blk(d)
    assert tuple(out.shape) == (B, 4 * 81, H, W)
    assert same_bits(out, ts.flow_corr_lookup(ts.flow_corr_pyramid(f1, f2, 4), d, 4, size=(H, W)))
    assert same_bits(ts.FlowCorrBlock(f1, f2, num_levels=2, radius=1)(d), ts.flow_corr_lookup(ts.flow_corr_pyramid(f1, f2, 2), d, 1))
    assert tuple(ts.FlowCorrBlock(f1, f2, num_levels=1, radius=0)(d).shape) == (B, 1, H, W)
    ref, tgt = ts.FlowCorrBlock.init_flow((B, C, H, W), _dev())
    assert ref.is_cuda and tuple(ref.shape) == (B, 2, H, W) and torch.equal(ref, tgt)
    xs, ys = torch.meshgrid(torch.arange(W, dtype=torch.float32), torch.arange(H, dtype=torch.float32), indexing="xy")
    assert torch.equal(ref[0, 0].cpu(), xs) and torch.equal(ref[0, 1].cpu(), ys)
    flow = gpu(c["coords"]) - ref
    assert same_bits(ts.FlowCorrBlock.init_flow((B, C, H, W), _dev(), flow_init=flow)[1], ref + flow)


def test_level_count_limit():
    """four levels (the reference's default) run in one launch; a fifth is refused by name: the 8-row patch pools no deeper"""
    f = gpu(torch.zeros(1, 2, 32, 32))
    assert len(ts.FlowCorrBlock(f, f, num_levels=4, radius=0).corr_pyramid) == 4
    with pytest.raises(ValueError, match="pools at most 4 levels"):
        ts.FlowCorrBlock(f, f, num_levels=5)
    with pytest.raises(ValueError, match="pools at most 4 levels"):
        ts.flow_corr_pyramid(f, f, 5)
    from temporalstereo_amd import _lib
    p = _lib.ptr
    assert _lib.lib().ts_flow_corr_pyramid_fwd(p(f), p(f), p(f), 1, 2, 32, 32, 5, None) == -3
    assert b"at most 4 levels" in _lib.lib().ts_last_error_string()


def test_refusals():
    B, C, H, W, L, r = SHAPES["a"]
    c = case("a")
    f1, f2, d = gpu(c["fmap1"]), gpu(c["fmap2"]), gpu(c["coords"])
    with pytest.raises(TypeError, match="fp32"):
        ts.FlowCorrBlock(f1.double(), f2.double(), num_levels=L)
    with pytest.raises(TypeError, match="fp32"):
        ts.FlowCorrBlock(f1, f2, num_levels=L)(d.half())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ts.FlowCorrBlock(f1.cpu(), f2.cpu(), num_levels=L)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ts.FlowCorrBlock(f1, f2, num_levels=L)(d.cpu())
    with pytest.raises(ValueError, match=r"must be \[B,C,H,W\]"):
        ts.FlowCorrBlock(f1[0], f2[0], num_levels=L)
    with pytest.raises(ValueError, match="differ in shape"):
        ts.FlowCorrBlock(f1, f2[:, :, :, :W - 1], num_levels=L)
    with pytest.raises(ValueError, match="does not match"):
        ts.FlowCorrBlock(f1, f2, num_levels=L)(d[:, :, :H - 1])
    with pytest.raises(ValueError, match=r"coords must be \[B,2,H,W\]"):
        ts.FlowCorrBlock(f1, f2, num_levels=L)(d[:, :1])
    with pytest.raises(ValueError, match="level 3 of a 8 x 11 map is 1 x 1"):
        ts.FlowCorrBlock(f1, f2)                                                              # the default four levels
    with pytest.raises(ValueError, match="level 0 of a 8 x 1 map"):
        ts.FlowCorrBlock(f1[..., :1], f2[..., :1], num_levels=1)
    with pytest.raises(ValueError, match="num_levels must be >= 1"):
        ts.FlowCorrBlock(f1, f2, num_levels=0)
    with pytest.raises(ValueError, match="radius must be >= 0"):
        ts.FlowCorrBlock(f1, f2, num_levels=L, radius=-1)
    pyr = ts.flow_corr_pyramid(f1, f2, 2)
    with pytest.raises(ValueError, match="radius must be >= 0"):
        ts.flow_corr_lookup(pyr, d, -1)
    with pytest.raises(ValueError, match="does not match size"):
        ts.flow_corr_lookup(pyr, d, 1, size=(H, W + 1))
    with pytest.raises(ValueError, match="no pyramid of a 8 x 11 map"):
        ts.flow_corr_lookup(pyr[:-B * H * W], d, 1)
