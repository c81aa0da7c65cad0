"""The 2-D inverse warp on the device (temporalstereo_amd.inverse_warp; csrc/inverse_warp.hip) against the reference's own runs recorded
in tests/golden/inverse_warp_*.npz (tools/gen_golden.py --only-warp) and, at shapes without a fixture and for the gradients, against
tests/warp_ref.py in fp64 on the CPU, which tests/test_inverse_warp_cpu.py pins to the same fixtures.

Bars, none taken from the code under test:
  forward     |hip - fp64 expectation| <= max(4 x dev32_64 of that case, 2^-22 max|img|), dev32_64 = max |fp32 run - fp64 run| of the
              reference (fixture) or of warp_ref on the CPU (no fixture).  dev32_64 is mostly coordinate rounding; a second, equally
              rounded evaluation with another contraction into fused multiply-adds can land about twice as far away, 4 leaves a factor
              of two.  flow_mask: equal.  Each case prints its ratio error / bar; with TS_WARP_PARITY_FILE set the line is appended to
              that file as well (that is how profiles/warp_parity.txt is made).
  nearest     bit-equal to the fp64 expectation cast to fp32 (values are copies; the motions stay a quarter pixel from a tie)
  edges       exact answers where the float sequence itself is exact (see test_edges_exact_answers)
  gradients   relative L2 error against fp64 autograd of warp_ref <= max(4 x the fp32 torch run's own relative L2 error, 1e-6)
"""
import functools
import os

import numpy as np
import pytest
import torch

import warp_ref as R
import temporalstereo_amd as ts
from compare import Parity, dev as _dev, gpu, rel_l2, same_bits
from temporalstereo_amd import _lib

pytestmark = pytest.mark.gpu

report = Parity("TS_WARP_PARITY_FILE").report
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODES = ("disparity", "flow", "depth")
PADS = ("zeros", "border", "reflection")
#        tag  B  C   H    W   Hi   Wi  K
SHAPES = {"a": (2, 3, 7, 37, 7, 37, 3),          # batch stride, odd C, ragged quad
          "b": (1, 5, 2, 66, 2, 66, 4),          # minimal H, two pixels past one wave
          "c": (2, 1, 9, 13, 5, 21, 3),          # image size differs from motion size, single channel
          "d": (1, 8, 33, 130, 33, 130, 3),      # more rows than one workgroup covers, 130 = 4 * 32 + 2 (no fixture: warp_ref)
          "e": (1, 17, 5, 4, 5, 4, 4)}           # channel-chunk tail, minimal quad width


def geometry(rng, B, H, W, kdim, small=False):
    """a camera (focal length 0.8 W, principal point at the centre) and a small rigid motion per batch element, depth in [1, 9]"""
    k = 0.05 if small else 1.0
    K, T = np.zeros((B, kdim, kdim)), np.zeros((B, 4, 4))
    for b in range(B):
        K[b] = np.eye(kdim)
        K[b, 0, 0] = K[b, 1, 1] = 0.8 * W
        K[b, 0, 2], K[b, 1, 2] = (W - 1) / 2.0, (H - 1) / 2.0
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        ang = k * rng.uniform(0.05, 0.2)
        S = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        T[b] = np.eye(4)
        T[b, :3, :3] = np.eye(3) + np.sin(ang) * S + (1 - np.cos(ang)) * S @ S
        t = rng.normal(size=3)
        T[b, :3, 3] = t / np.linalg.norm(t) * k * rng.uniform(0.1, 0.4)
    f = lambda a: torch.from_numpy(a).float()
    K32 = f(K)
    return K32, torch.inverse(K32[:, :3, :3]).contiguous(), f(T), f(rng.uniform(1.0, 9.0, size=(B, 1, H, W)))


@functools.lru_cache(maxsize=None)
def case(tag):
    """inputs of a shape (CPU, fp32), the reference's dev32_64 where a fixture has them"""
    B, C, H, W, Hi, Wi, kdim = SHAPES[tag]
    path = os.path.join(GOLDEN, "inverse_warp_%s.npz" % tag)
    if os.path.exists(path):
        g = dict(np.load(path))
        c = {k: torch.from_numpy(g[k]) for k in ("img", "motion_disparity", "motion_flow", "motion_depth", "K", "inv_K", "T")}
        c["dev"] = {k[4:]: float(v) for k, v in g.items() if k.startswith("dev_")}
        assert tuple(c["img"].shape) == (B, C, Hi, Wi) and tuple(c["motion_flow"].shape) == (B, 2, H, W)
        return c
    rng = np.random.default_rng(20260 + ord(tag))
    f = lambda a: torch.from_numpy(a).float()
    c = dict(img=f(rng.normal(size=(B, C, Hi, Wi))), motion_disparity=f(rng.uniform(-0.75, 0.75, size=(B, 1, H, W)) * W),
             motion_flow=f(rng.uniform(-0.75, 0.75, size=(B, 2, H, W)) * np.array([W, H]).reshape(1, 2, 1, 1)), dev={})
    for attempt in range(200):        # the generator's rule: no projected pixel within 1e-4 px of a flow_mask bound, fp32 mask == fp64 mask
        K, iK, T, depth = geometry(np.random.default_rng(30260 + 1000 * ord(tag) + attempt), B, H, W, kdim)
        s32, s64 = R.project(depth, K, iK, T), R.project(depth.double(), K.double(), iK.double(), T.double())
        q = s64["src_pixel_coord"]
        gap = min(q[:, 0].abs().min(), (q[:, 0] - (W - 1)).abs().min(), q[:, 1].abs().min(), (q[:, 1] - (H - 1)).abs().min())
        if gap > 1e-4 and torch.equal(s32["flow_mask"], s64["flow_mask"]):
            break
    assert gap > 1e-4 and torch.equal(s32["flow_mask"], s64["flow_mask"])
    c.update(motion_depth=depth, K=K, inv_K=iK, T=T)
    return c


def geo_of(c, mode, dtype=torch.float32):
    return tuple(c[k].to(dtype) for k in ("K", "inv_K", "T")) if mode == "depth" else (None, None, None)


def expectation(img, motion, mode, geo, interp, pad):
    """fp64 expectation and the fp32 run's own deviation from it (per output), both by warp_ref on the CPU"""
    g64 = tuple(None if t is None else t.double() for t in geo)
    o64, s64 = R.inverse_warp(img.double(), motion.double(), mode, *g64, interp, pad)
    o32, s32 = R.inverse_warp(img, motion, mode, *geo, interp, pad)
    dev = {"out": float((o32.double() - o64).abs().max())}
    for k in s64:
        if k != "flow_mask":
            dev[k] = float((s32[k].double() - s64[k]).abs().max())
    return o64, s64, dev


def check_bar(name, got, want64, dev, floor):
    err = float((got.detach().cpu().double() - want64).abs().max())
    bar = max(4.0 * dev, floor)
    report("%-44s err %.3e  dev32_64 %.3e  bar %.3e  err/bar %.3f" % (name, err, dev, bar, err / bar))
    assert err <= bar, "%s: error %.3e above max(4 x %.3e, %.3e)" % (name, err, dev, floor)


def hip_warp(c_img, motion, mode, geo, interp="bilinear", pad="zeros", output_all=False):
    K, iK, T = (gpu(t) for t in geo)
    return ts.inverse_warp(gpu(c_img), gpu(motion), mode, K, iK, T, interp, pad, output_all=output_all)


# ------------------------------------------------------------------------------------------------------------------ 1. forward
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tag", sorted(SHAPES))
def test_forward_against_the_reference(tag, mode, pad):
    c = case(tag)
    img, motion, geo = c["img"], c["motion_" + mode], geo_of(c, mode)
    want, side, own = expectation(img, motion, mode, geo, "bilinear", pad)
    dev = c["dev"].get("%s_%s" % (mode, pad), own["out"])                      # the reference's own where a fixture holds it
    floor = 2.0 ** -22 * float(img.abs().max())
    got, out = hip_warp(img, motion, mode, geo, "bilinear", pad, output_all=True)
    check_bar("fwd %s %-9s %-10s" % (tag, mode, pad), got, want, dev, floor)
    if mode != "depth":
        assert out == {}
        return
    assert sorted(out) == sorted(side)
    assert out["flow_mask"].dtype == torch.bool and torch.equal(out["flow_mask"].cpu(), side["flow_mask"])
    for k in ("triangular_depth", "src_pixel_coord", "optical_flow", "homo_points_3d"):
        assert out[k].shape == side[k].shape and out[k].dtype == torch.float32
        check_bar("fwd %s %-9s %-10s %s" % (tag, mode, pad, k), out[k], side[k], c["dev"].get("side_" + k, own[k]), 0.0)


# ------------------------------------------------------------------------------------------------------------------ 2. nearest
def quarter_motion(rng, B, n, H, W):
    """an integer plus a fraction from {0, 0.25, 0.75}: exact in fp32, never within a quarter pixel of a rounding tie"""
    size = np.array([W, H][:n]).reshape(1, n, 1, 1)
    whole = np.floor(rng.uniform(-0.6, 0.6, size=(B, n, H, W)) * size)
    return torch.from_numpy(whole + rng.choice([0.0, 0.25, 0.75], size=(B, n, H, W))).float()


@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("mode", ("disparity", "flow"))
@pytest.mark.parametrize("tag", ("a", "d", "e"))
def test_nearest_copies_the_right_pixel(tag, mode, pad):
    B, C, H, W, Hi, Wi, _ = SHAPES[tag]
    rng = np.random.default_rng(511 + ord(tag))
    img = case(tag)["img"]
    motion = quarter_motion(rng, B, 1 if mode == "disparity" else 2, H, W)
    want = R.inverse_warp(img.double(), motion.double(), mode, None, None, None, "nearest", pad)[0].float()
    got = hip_warp(img, motion, mode, (None, None, None), "nearest", pad)
    assert same_bits(got.cpu(), want)
    assert float((want != 0).float().mean()) > 0.25                           # the case does sample the image


# ------------------------------------------------------------------------------------------------------------------ 3. edges
def test_edges_exact_answers():
    """C = 3, 6 x 19.  Every pixel is sent to one of X in {0, W-1, -1, W, x + 1e9, x - 1e9} and, in flow mode, independently to one
    of Y in {0, H-1, -1, H, y + 1e9, y - 1e9}: all 36 pairs occur.
      border   exactly the pixel at the clipped position, for every pair (0 and size - 1 survive the normalise / un-normalise round
               trip exactly, everything outside is clipped onto them);
      zeros    exactly 0 wherever X is -1, W or +-1e9, or Y is H or +-1e9 (in disparity mode: wherever X is): the fp32 round trip
               gives -1.0000005 for X = -1 at W = 19 and exactly W and H for X = W and Y = H, so both taps of that axis lie
               outside; exactly the corner pixel where X in {0, W-1} and Y in {0, H-1}.
    Y = -1 alone is not exact at H = 6: the round trip gives -0.99999994 (in the reference's fp32 run too), so row 0 keeps a weight
    of 6e-8.  Those pixels (with X inside), and every case as a whole, are held to the forward bar against the fp64 expectation."""
    B, C, H, W = 1, 3, 6, 19
    rng = np.random.default_rng(77)
    img = torch.from_numpy(rng.normal(size=(B, C, H, W))).float()
    p = np.arange(H * W)
    kx, ky = (p % 6).reshape(H, W), ((p // 6) % 6).reshape(H, W)
    assert len(set(zip(kx.ravel().tolist(), ky.ravel().tolist()))) == 36
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    tx = np.choose(kx, [0 * xs, 0 * xs + W - 1, 0 * xs - 1, 0 * xs + W, xs, xs]).astype(np.float64)
    ty = np.choose(ky, [0 * ys, 0 * ys + H - 1, 0 * ys - 1, 0 * ys + H, ys, ys]).astype(np.float64)
    mx = tx - xs + np.choose(kx, [0, 0, 0, 0, 1e9, -1e9])
    my = ty - ys + np.choose(ky, [0, 0, 0, 0, 1e9, -1e9])
    clip_x = np.choose(kx, [0, W - 1, 0, W - 1, W - 1, 0])
    clip_y = np.choose(ky, [0, H - 1, 0, H - 1, H - 1, 0])
    flow = torch.from_numpy(np.stack([mx, my])[None]).float()
    disp = flow[:, :1].contiguous()
    floor = 2.0 ** -22 * float(img.abs().max())
    none = (None, None, None)

    got = hip_warp(img, flow, "flow", none, "bilinear", "border").cpu()
    assert torch.equal(got[0], img[0][:, torch.from_numpy(clip_y), torch.from_numpy(clip_x)])

    got = hip_warp(img, flow, "flow", none, "bilinear", "zeros").cpu()
    far = torch.from_numpy((kx >= 2) | (ky >= 3))                         # X in {-1, W, +-1e9} or Y in {H, +-1e9}
    corner = torch.from_numpy((kx < 2) & (ky < 2))
    assert far.any() and corner.any()
    assert (got[0][:, far] == 0).all()
    assert torch.equal(got[0][:, corner], img[0][:, torch.from_numpy(clip_y), torch.from_numpy(clip_x)][:, corner])
    want, _, own = expectation(img, flow, "flow", none, "bilinear", "zeros")
    check_bar("edges flow zeros", got, want, own["out"], floor)

    for pad in ("zeros", "border"):
        got = hip_warp(img, disp, "disparity", none, "bilinear", pad).cpu()
        want, _, own = expectation(img, disp, "disparity", none, "bilinear", pad)
        check_bar("edges disparity %s" % pad, got, want, own["out"], floor)
        if pad == "zeros":
            assert (got[0][:, torch.from_numpy(kx >= 2)] == 0).all()          # X in {-1, W, +-1e9}, whatever the row
        else:
            assert torch.equal(got[0][:, 0], img[0][:, 0, torch.from_numpy(clip_x[0])])     # row 0: Y = 0 is exact, the clipped column's pixel


@pytest.mark.parametrize("mode", ("disparity", "flow"))
def test_reflection_over_several_periods(mode):
    B, C, H, W = 1, 3, 6, 19
    rng = np.random.default_rng(78)
    img = torch.from_numpy(rng.normal(size=(B, C, H, W))).float()
    n = 1 if mode == "disparity" else 2
    size = np.array([W, H][:n]).reshape(1, n, 1, 1)
    far = rng.choice([2.5, -2.5, 7.0, -7.0], size=(B, n, H, W)) * size
    motion = torch.from_numpy(far + rng.uniform(-0.4, 0.4, size=(B, n, H, W))).float()
    want, _, own = expectation(img, motion, mode, (None, None, None), "bilinear", "reflection")
    got = hip_warp(img, motion, mode, (None, None, None), "bilinear", "reflection")
    check_bar("reflection periods %s" % mode, got, want, own["out"], 2.0 ** -22 * float(img.abs().max()))


# ------------------------------------------------------------------------------------------------------------------ 4. integers
def test_integer_disparities_shift_the_image():
    B, C, H, W = 2, 3, 7, 37
    rng = np.random.default_rng(79)
    img = torch.from_numpy(rng.normal(size=(B, C, H, W))).float()
    d = torch.from_numpy(rng.integers(-W, W + 1, size=(B, 1, H, W))).float()
    src = torch.arange(W).view(1, 1, 1, W) + d.long()
    inside = (src >= 0) & (src < W)
    want = torch.gather(img, 3, src.clamp(0, W - 1).expand(B, C, H, W)) * inside
    got = hip_warp(img, d, "disparity", (None, None, None)).cpu()
    err = float((got - want).abs().max())
    print("integer disparities: err %.3e, bar %.3e" % (err, 2.0 ** -20 * float(img.abs().max())))
    assert err <= 2.0 ** -20 * float(img.abs().max())


# ------------------------------------------------------------------------------------------------------------------ 5. gradients
def torch_grads(img, motion, mode, geo, interp, pad, gout, dtype, need_motion):
    cast = lambda t: None if t is None else t.to(dtype)
    i = img.detach().clone().to(dtype).requires_grad_(True)
    m = motion.detach().clone().to(dtype).requires_grad_(need_motion)
    out = R.inverse_warp(i, m, mode, *(cast(t) for t in geo), interp, pad)[0]
    out.backward(gout.to(dtype))
    return i.grad, (m.grad if need_motion else None)


def hip_grads(img, motion, mode, geo, interp, pad, gout, need_motion):
    i = gpu(img).detach().clone().requires_grad_(True)
    m = gpu(motion).detach().clone().requires_grad_(need_motion)
    K, iK, T = (gpu(t) for t in geo)
    ts.inverse_warp(i, m, mode, K, iK, T, interp, pad).backward(gpu(gout))
    return i.grad, (m.grad if need_motion else None)


def fraction_motion(rng, B, n, H, W):
    """an integer plus a fraction from [0.1, 0.9]: the derivative with respect to the position is discontinuous at integers"""
    size = np.array([W, H][:n]).reshape(1, n, 1, 1)
    whole = np.floor(rng.uniform(-0.75, 0.75, size=(B, n, H, W)) * size)
    return torch.from_numpy(whole + rng.uniform(0.1, 0.9, size=(B, n, H, W))).float()


def grad_case(tag, mode, rng):
    """(img, motion, geo, keep): keep is None where the fractions were drawn, else the pixels whose fp64 position stays 0.01 away
    from every integer (depth mode and the differing-size case cannot draw their fractions)"""
    B, C, H, W, Hi, Wi, _ = SHAPES[tag]
    c = case(tag)
    geo = geo_of(c, mode)
    if mode == "depth":
        motion = c["motion_depth"]
    else:
        motion = fraction_motion(rng, B, 1 if mode == "disparity" else 2, H, W)
    keep = None
    if mode == "depth" or (Hi, Wi) != (H, W):
        ix, iy = R.positions(motion.double(), mode, (Hi, Wi), *(None if t is None else t.double() for t in geo))
        near = lambda v: (v - v.round()).abs() < 0.01
        keep = ~((near(ix) | near(iy)) if mode != "disparity" else near(ix))
        assert float((~keep).float().mean()) < 0.10
        keep = keep.unsqueeze(1).double()
    return c["img"], motion, geo, keep


GRAD_CASES = [("a", m, p) for m in MODES for p in PADS] + [("c", "disparity", "zeros"), ("d", "flow", "border"), ("e", "depth", "reflection")]


@pytest.mark.parametrize("tag,mode,pad", GRAD_CASES)
def test_gradients_against_fp64_autograd(tag, mode, pad):
    rng = np.random.default_rng(900 + ord(tag) + 7 * MODES.index(mode) + 31 * PADS.index(pad))
    img, motion, geo, keep = grad_case(tag, mode, rng)
    B, C, H, W = SHAPES[tag][:4]
    gout = torch.from_numpy(rng.normal(size=(B, C, H, W))).float()
    gi64, gm64 = torch_grads(img, motion, mode, geo, "bilinear", pad, gout, torch.float64, True)
    gi32, gm32 = torch_grads(img, motion, mode, geo, "bilinear", pad, gout, torch.float32, True)
    bar_i = max(4 * rel_l2(gi32, gi64), 1e-6)
    bar_m = max(4 * rel_l2(gm32, gm64, keep=keep), 1e-6)
    first = None
    for run in range(2 if (tag, mode, pad) == ("a", "flow", "zeros") else 1):
        gi, gm = hip_grads(img, motion, mode, geo, "bilinear", pad, gout, True)
        ei, em = rel_l2(gi, gi64), rel_l2(gm, gm64, keep=keep)
        report("grad %s %-9s %-10s img %.3e (bar %.3e, ratio %.3f)  motion %.3e (bar %.3e, ratio %.3f)"
               % (tag, mode, pad, ei, bar_i, ei / bar_i, em, bar_m, em / bar_m))
        assert gm.shape == motion.shape and ei <= bar_i and em <= bar_m
        if first is not None:
            assert same_bits(gm, first)                   # the motion gradient is a gather: deterministic
        first = gm.clone()


@pytest.mark.parametrize("tag,mode,pad", [("a", "disparity", "zeros"), ("a", "flow", "border"), ("e", "flow", "reflection"),
                                          ("d", "disparity", "reflection")])
def test_nearest_gradient_of_the_image(tag, mode, pad):
    B, C, H, W = SHAPES[tag][:4]
    rng = np.random.default_rng(950 + ord(tag))
    img = case(tag)["img"]
    motion = quarter_motion(rng, B, 1 if mode == "disparity" else 2, H, W)
    gout = torch.from_numpy(rng.normal(size=(B, C, H, W))).float()
    none = (None, None, None)
    gi64, _ = torch_grads(img, motion, mode, none, "nearest", pad, gout, torch.float64, False)
    gi32, _ = torch_grads(img, motion, mode, none, "nearest", pad, gout, torch.float32, False)
    gi, _ = hip_grads(img, motion, mode, none, "nearest", pad, gout, False)
    bar = max(4 * rel_l2(gi32, gi64), 1e-6)
    report("grad nearest %s %-9s %-10s img %.3e (bar %.3e)" % (tag, mode, pad, rel_l2(gi, gi64), bar))
    assert rel_l2(gi, gi64) <= bar
    gi, gm = hip_grads(img, motion, mode, none, "nearest", pad, gout, True)
    assert rel_l2(gi, gi64) <= bar and gm.shape == motion.shape and not gm.any()     # a step function of the motion


def test_image_only_gradient_splits_the_channels():
    """without a motion gradient the backward launch splits the channel range over the grid (C = 17: a ragged last slice)"""
    img, motion, geo, _ = grad_case("e", "flow", np.random.default_rng(960))
    gout = torch.from_numpy(np.random.default_rng(961).normal(size=SHAPES["e"][:4])).float()
    gi64, _ = torch_grads(img, motion, "flow", geo, "bilinear", "zeros", gout, torch.float64, False)
    gi32, _ = torch_grads(img, motion, "flow", geo, "bilinear", "zeros", gout, torch.float32, False)
    gi, gm = hip_grads(img, motion, "flow", geo, "bilinear", "zeros", gout, False)
    assert gm is None and rel_l2(gi, gi64) <= max(4 * rel_l2(gi32, gi64), 1e-6)


# ------------------------------------------------------------------------------------------------------------------ 6. contracts
def test_forward_is_bit_identical_and_takes_views():
    c = case("a")
    img, flow = gpu(c["img"]), gpu(c["motion_flow"])
    one = ts.inverse_warp(img, flow, "flow", padding_mode="border")
    assert torch.is_tensor(one) and same_bits(one, ts.inverse_warp(img, flow, "flow", padding_mode="border"))
    wide_img = torch.zeros(2, 3, 7, 40, device=_dev())
    wide_img[..., :37] = img
    tall_flow = flow.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert not wide_img[..., :37].is_contiguous() and not tall_flow.is_contiguous()
    assert same_bits(one, ts.inverse_warp(wide_img[..., :37], tall_flow, "flow", padding_mode="border"))


def test_output_all_returns_the_reference_structure():
    c = case("c")
    for mode in MODES:
        K, iK, T = (gpu(t) for t in geo_of(c, mode))
        res = ts.inverse_warp(gpu(c["img"]), gpu(c["motion_" + mode]), mode, K, iK, T, output_all=True)
        assert isinstance(res, tuple) and len(res) == 2 and torch.is_tensor(res[0]) and isinstance(res[1], dict)
        assert (sorted(res[1]) == ["flow_mask", "homo_points_3d", "optical_flow", "src_pixel_coord", "triangular_depth"]) == (mode == "depth")
        assert torch.is_tensor(ts.inverse_warp(gpu(c["img"]), gpu(c["motion_" + mode]), mode, K, iK, T))
    # inv_K=None: torch.inverse(K[:, :3, :3]) on the device, as in project_to_3d; the side outputs carry no gradient
    depth = gpu(c["motion_depth"]).detach().clone().requires_grad_(True)
    out, side = ts.inverse_warp(gpu(c["img"]), depth, "depth", gpu(c["K"]), None, gpu(c["T"]), output_all=True)
    want = R.inverse_warp(c["img"].double(), c["motion_depth"].double(), "depth", c["K"].double(), None, c["T"].double())[0]
    assert float((out.detach().cpu().double() - want).abs().max()) < 1e-3
    assert out.requires_grad and not any(v.requires_grad for v in side.values())
    proj = ts.project_to_3d(gpu(c["motion_depth"]), gpu(c["K"]), gpu(c["inv_K"]), gpu(c["T"]))
    full = ts.inverse_warp(gpu(c["img"]), gpu(c["motion_depth"]), "depth", gpu(c["K"]), gpu(c["inv_K"]), gpu(c["T"]), output_all=True)[1]
    for k in ("triangular_depth", "optical_flow"):                        # the shared projection: the two entries agree bit for bit
        assert same_bits(proj[k], full[k]), k
    assert torch.equal(proj["flow_mask"], full["flow_mask"])


def test_a_launch_plan_replays_the_warp():
    c = case("d")
    img, depth = gpu(c["img"]), gpu(c["motion_depth"])
    K, iK, T = (gpu(t) for t in geo_of(c, "depth"))
    with _lib.Recorder() as rec:
        out, side = ts.inverse_warp(img, depth, "depth", K, iK, T, padding_mode="reflection", output_all=True)
    assert [n for n, _ in rec.log] == ["ts_inverse_warp_fwd"]
    torch.cuda.synchronize()
    floats = [out] + [side[k] for k in ("triangular_depth", "src_pixel_coord", "optical_flow", "homo_points_3d")]
    want = [t.clone() for t in floats]
    for t in floats:
        t.fill_(float("nan"))
    rec.run()
    torch.cuda.synchronize()
    for t, w in zip(floats, want):
        assert same_bits(t, w)
    # refilled inputs: the replay reads the same buffers
    img.copy_(gpu(torch.from_numpy(np.random.default_rng(5).normal(size=tuple(img.shape))).float()))
    rec.run()
    torch.cuda.synchronize()
    assert same_bits(out, ts.inverse_warp(img, depth, "depth", K, iK, T, padding_mode="reflection"))


def test_refusals_carry_the_library_message():
    c = case("a")
    img, disp = gpu(c["img"]), gpu(c["motion_disparity"])
    with pytest.raises(RuntimeError, match="bicubic"):
        ts.inverse_warp(img, disp, interpolate_mode="bicubic")
    with pytest.raises(RuntimeError, match=">= 2"):
        ts.inverse_warp(img[:, :, :, :1].contiguous(), disp)
    with pytest.raises(RuntimeError, match=">= 2"):
        ts.inverse_warp(img, disp[:, :, :1].contiguous())
