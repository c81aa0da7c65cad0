"""Training-frame augmentation on the device (temporalstereo_amd/augment.py, csrc/augment.hip) against the reference's own
do_transform runs recorded in tests/golden/augment_*.npz (tools/gen_golden.py --only-augment) and, at full size, against the numpy
restatement of tests/augment_ref.py, which tests/test_augment_cpu.py pins to the same fixtures.

Bars, none taken from the code under test:
  - `color` everywhere and `color_aug` outside the union of the occlusion rectangles: torch.equal with the reference's tensors.  The
    rectangles' pixels are the ONLY ones left out of that comparison.
  - inside the rectangles the reference's numpy noise stream is not reproduced; the layout is exact (>= 99.9 % of the pixels inside
    the union differ from the un-occluded result, none outside does), and per channel, on n >= 5000 samples, v * std[c] + mean[c] has
    |mean| <= 5 * 0.1 / sqrt(n), a standard deviation within 5 % of 0.1 and a share beyond +-0.2 within 0.0455 +- 0.01 (the two-sigma
    tail of a normal distribution).
"""
import os

import numpy as np
import pytest
import torch

import augment_ref as R
from compare import dev as _dev, gpu, same_bits
from temporalstereo_amd import _lib, augment as ag, preprocess as pp

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ("augment_ops", "augment_orders", "augment_chain", "augment_occlusion", "augment_large", "augment_identity")
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def fixture_rects(g, b):
    return [tuple(int(v) for v in q) for q in g["rects"][b][:int(g["nrect"][b])]]


def fixture_aug(g, seed=99, rects=True, device=None):
    """the Augmentation of a fixture's recorded parameters"""
    colour = bool((g["order"] != R.NONE).any() or (g["gamma"] != 1.0).any() or not np.array_equal(g["stage_l"], g["left"]))
    B = g["left"].shape[0]
    rows = [[None] * B for _ in range(2)]
    for e in range(2):
        for b in range(B):
            d = dict(order=[int(o) for o in g["order"][e, b]], seed=seed + 1000 * e + b)
            d.update(zip(("brightness", "contrast", "saturation", "hue"), (float(v) for v in g["factors"][e, b])))
            if colour:
                d["gamma"] = float(g["gamma"][e, b])
            if e == 1 and rects:
                d["rects"] = fixture_rects(g, b)
            rows[e][b] = d
    return ag.Augmentation.from_values(rows, crop=g["crop"], device=_dev() if device is None else device)


@pytest.mark.parametrize("layout", ("HWC", "CHW"))
@pytest.mark.parametrize("name", CASES)
def test_fixture_bit_equal_outside_rectangles(name, layout):
    g = load(name)
    size = tuple(int(v) for v in g["size"])
    L, Rt = gpu(g["left"]), gpu(g["right"])
    if layout == "CHW":
        L, Rt = L.permute(0, 3, 1, 2).contiguous(), Rt.permute(0, 3, 1, 2).contiguous()
    r = ag.augment_frames(L, Rt, fixture_aug(g), size, layout=layout)
    B = g["left"].shape[0]
    for s in "lr":
        assert same_bits(r["color_" + s].cpu(), torch.from_numpy(g["color_" + s])), (name, s, "color")
        got, exp = r["color_aug_" + s].cpu().numpy(), g["aug_" + s]
        for b in range(B):
            keep = ~R.rect_mask(fixture_rects(g, b) if s == "r" else [], size)
            assert keep.all() or s == "r"
            bad = got[b].view(np.int32)[:, keep] != exp[b].view(np.int32)[:, keep]
            assert not bad.any(), "%s %s image %d eye %s: %d of %d values differ" % (name, layout, b, s, bad.sum(), bad.size)


@pytest.mark.parametrize("name", ("augment_occlusion", "augment_large"))
def test_rectangle_layout_is_exact(name):
    g = load(name)
    size = tuple(int(v) for v in g["size"])
    L, Rt = gpu(g["left"]), gpu(g["right"])
    with_r = ag.augment_frames(L, Rt, fixture_aug(g), size)
    without = ag.augment_frames(L, Rt, fixture_aug(g, rects=False), size)
    assert same_bits(with_r["color_aug_l"], without["color_aug_l"]) and same_bits(with_r["color_r"], without["color_r"])
    for b in range(g["left"].shape[0]):
        inside = R.rect_mask(fixture_rects(g, b), size)
        diff = (with_r["color_aug_r"][b] != without["color_aug_r"][b]).cpu().numpy()
        assert not diff[:, ~inside].any(), (name, b)
        assert diff[:, inside].mean() >= 0.999, (name, b, diff[:, inside].mean())


def test_noise_statistics():
    g = load("augment_large")
    size = tuple(int(v) for v in g["size"])
    r = ag.augment_frames(gpu(g["left"]), gpu(g["right"]), fixture_aug(g), size)["color_aug_r"][0].cpu().numpy().astype(np.float64)
    inside = R.rect_mask(fixture_rects(g, 0), size)
    n = int(inside.sum())
    assert n >= 5000
    for c in range(3):
        v = r[c][inside] * STD[c] + MEAN[c]
        tail = float((np.abs(v) > 0.2).mean())
        print("channel %d: n %d mean %.5f std %.5f tail %.4f" % (c, n, v.mean(), v.std(), tail))
        assert abs(v.mean()) <= 5 * 0.1 / np.sqrt(n), (c, v.mean())
        assert abs(v.std() - 0.1) <= 0.05 * 0.1, (c, v.std())
        assert abs(tail - 0.0455) <= 0.01, (c, tail)
    # the channels and the two rectangles hold different draws
    assert not np.array_equal(r[0][inside], r[1][inside])


def test_noise_depends_on_the_seed_and_on_nothing_else():
    g = load("augment_occlusion")
    size = tuple(int(v) for v in g["size"])
    H, W = size
    L, Rt = gpu(g["left"]), gpu(g["right"])
    a = ag.augment_frames(L, Rt, fixture_aug(g, seed=5), size)["color_aug_r"]
    again = ag.augment_frames(L, Rt, fixture_aug(g, seed=5), size)["color_aug_r"]
    other = ag.augment_frames(L, Rt, fixture_aug(g, seed=6), size)["color_aug_r"]
    assert same_bits(a, again)
    for b in range(3):
        inside = torch.from_numpy(R.rect_mask(fixture_rects(g, b), size)).to(_dev())
        assert (a[b][:, inside] != other[b][:, inside]).float().mean() > 0.999
        assert same_bits(a[b][:, ~inside], other[b][:, ~inside])
    # image 2 alone (B=1), and the same table row and frames as image 1 of B=3, into a strided out
    full = fixture_aug(g, seed=5, device="cpu")
    rows = lambda e, b: dict(order=[int(o) for o in full.order[e, b]], brightness=full.factors[e, b, 0], contrast=full.factors[e, b, 1],
                             saturation=full.factors[e, b, 2], hue=full.factors[e, b, 3], gamma=float(g["gamma"][e, b]),
                             rects=full.rects[e][b], seed=int(full.seeds[e, b]))
    alone = ag.Augmentation.from_values([[rows(0, 2)], [rows(1, 2)]], crop=[full.crop[2]], device=_dev())
    one = ag.augment_frames(L[2:3], Rt[2:3], alone, size)["color_aug_r"]
    assert same_bits(one[0], a[2])
    moved = ag.Augmentation.from_values([[rows(0, 0), rows(0, 2), rows(0, 1)], [rows(1, 0), rows(1, 2), rows(1, 1)]],
                                        crop=[full.crop[0], full.crop[2], full.crop[1]], device=_dev())
    assert np.array_equal(moved.table_host()[:, 1], full.table_host()[:, 2])
    idx = torch.tensor([0, 2, 1], device=_dev())
    big_l = torch.full((3, 2, 3, H, W), float("nan"), device=_dev())
    big_r = torch.full((3, 2, 3, H, W), float("nan"), device=_dev())
    res = ag.augment_frames(L[idx].contiguous(), Rt[idx].contiguous(), moved, size, out=(big_l[:, 1], big_r[:, 1]))
    assert res["color_aug_r"].data_ptr() == big_r[:, 1].data_ptr() and res["color_aug_r"].stride(0) == 2 * 3 * H * W
    assert same_bits(big_r[1, 1], a[2]) and same_bits(big_r[0, 1], a[0]) and same_bits(big_r[2, 1], a[1])
    assert bool(torch.isnan(big_r[:, 0]).all()) and bool(torch.isnan(big_l[:, 0]).all())
    left = ag.augment_frames(L, Rt, fixture_aug(g, seed=5), size)["color_aug_l"]
    assert same_bits(big_l[1, 1], left[2])


@pytest.mark.parametrize("layout", ("HWC", "CHW"))
def test_identity_equals_prepare_frames(layout):
    g = load("augment_chain")
    size = tuple(int(v) for v in g["size"])
    L, Rt = gpu(g["left"]), gpu(g["right"])
    if layout == "CHW":
        L, Rt = L.permute(0, 3, 1, 2).contiguous(), Rt.permute(0, 3, 1, 2).contiguous()
    crops = [tuple(int(v) for v in c) for c in g["crop"]]
    want = pp.prepare_frames(L, Rt, size=size, crop=crops, layout=layout)
    got = ag.augment_frames(L, Rt, ag.Augmentation.identity(len(crops), crop=crops, device=_dev()), size, layout=layout)
    assert set(got) == set(want)
    for k in want:
        assert same_bits(got[k], want[k]) and got[k].stride() == want[k].stride(), k
    one = ag.augment_frames(L[1], None, ag.Augmentation.identity(1, crop=crops[1:], eyes=1, device=_dev()), size, layout=layout, color=False)
    assert set(one) == {"color_aug_l"} and same_bits(one["color_aug_l"], want["color_aug_l"][1])


@pytest.mark.parametrize("seed,p_color", ((11, 1.0), (12, 1.0), (13, 0.5)))
def test_full_size_equals_the_restatement(seed, p_color):
    """540 x 960 frames, a 512 x 960 window (the reference's SceneFlow training size), B=4, drawn parameters: the full-frame contrast
    reduction across many workgroups."""
    Hs, Ws, H, W, B = 540, 960, 512, 960, 4
    rs = np.random.RandomState(seed)
    frames = []
    for _ in range(2):
        tiles = rs.randint(0, 256, size=(B, Hs // 4, Ws // 4, 3)).astype(np.uint8)
        img = np.repeat(np.repeat(tiles, 4, axis=1), 4, axis=2)
        img ^= rs.randint(0, 8, size=img.shape).astype(np.uint8)                      # structure plus fine noise
        img[:, :8] = img[:, :8, :, :1]                                                # greys
        frames.append(np.ascontiguousarray(img))
    aug = ag.draw_augmentation(B, (Hs, Ws), (H, W), seed=seed, p_color=p_color, device=_dev())
    r = ag.augment_frames(gpu(frames[0]), gpu(frames[1]), aug, (H, W))
    n_contrast = 0
    for e, s in enumerate("lr"):
        got_c, got_a = r["color_" + s].cpu().numpy(), r["color_aug_" + s].cpu().numpy()
        for b in range(B):
            order = [int(o) for o in aug.order[e, b]]
            n_contrast += R.CONTRAST in order
            table = aug.gamma_tables[e, b] if aug.gamma_on[e, b] else None
            _, color, exp = R.frame(frames[e][b], order, aug.factors[e, b], int(aug.hue_shift[e, b]), table,
                                    tuple(int(v) for v in aug.crop[b]), (H, W), MEAN, STD)
            assert np.array_equal(got_c[b].view(np.int32), color.view(np.int32)), (seed, s, b, "color")
            keep = ~R.rect_mask(aug.rects[e][b], (H, W))
            bad = got_a[b].view(np.int32)[:, keep] != exp.view(np.int32)[:, keep]
            assert not bad.any(), "seed %d eye %s image %d (order %s): %d of %d values differ" % (seed, s, b, order, bad.sum(), bad.size)
    assert n_contrast >= 2


def _train_inputs(B=2, Hs=37, Ws=57):
    g = load("augment_chain")
    rs = np.random.RandomState(3)
    raw = rs.randint(0, 65536, size=(B, Hs, Ws)).astype(np.uint16)
    raw[rs.uniform(size=raw.shape) < 0.3] = 0
    kn = torch.tensor([[0.58, 0, 0.5, 0], [0, 1.92, 0.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=torch.float32, device=_dev())
    return g, gpu(g["left"]), gpu(g["right"]), kn, gpu(raw.view(np.int16)), torch.full((B,), 0.54, device=_dev())


def test_prepare_train_batch():
    g, L, Rt, kn, raw, base = _train_inputs()
    size = tuple(int(v) for v in g["size"])
    H, W = size
    crops = [tuple(int(v) for v in c) for c in g["crop"]]
    aug = fixture_aug(g)
    batch = ag.prepare_train_batch(L, Rt, kn, base, size, aug, disp_gt_raw=raw)
    ref = pp.prepare_batch(L, Rt, kn, base, size, crop=crops, k_size=(37, 57), disp_gt_raw=raw)
    assert set(batch) == set(ref)
    for k in ref:
        if k[0] == "disp_gt":
            continue
        assert batch[k].shape == ref[k].shape and batch[k].stride() == ref[k].stride() and batch[k].dtype == ref[k].dtype, k
        if k[0] != "color_aug":
            assert same_bits(batch[k], ref[k]), k
    for s in "lr":
        assert same_bits(batch[("color_aug", 0, s)].cpu(), torch.from_numpy(g["aug_" + s])), s
    full = pp.disp_from_uint16(raw)
    assert batch[("disp_gt", 0, "l")].shape == (2, 1, H, W) and batch[("disp_gt", 0, "l")].is_contiguous()
    for b, (ch, cw) in enumerate(crops):
        assert same_bits(batch[("disp_gt", 0, "l")][b], full[b, :, ch:ch + H, cw:cw + W]), b
    d, valid = ag.disp_window_from_uint16(raw, aug, size, with_valid=True)
    assert same_bits(d, batch[("disp_gt", 0, "l")]) and torch.equal(valid, d > 0)
    # identity parameters: prepare_batch's training form, value for value
    ident = ag.prepare_train_batch(L, Rt, kn, base, size, ag.Augmentation.identity(2, crop=crops, device=_dev()), disp_gt_raw=raw)
    for k in ref:
        if k[0] != "disp_gt":
            assert same_bits(ident[k], ref[k]), k


def test_prepare_train_batch_is_captured_and_replays_on_a_refilled_table():
    g, L, Rt, kn, raw, base = _train_inputs()
    size = tuple(int(v) for v in g["size"])
    first = ag.draw_augmentation(2, (37, 57), size, seed=1, p_color=1.0, p_occlusion=1.0, patch_w=(5, 20), patch_h=(5, 12), device=_dev())
    second = fixture_aug(g, seed=77)
    want = ag.prepare_train_batch(L, Rt, kn, base, size, second, disp_gt_raw=raw)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            batch = ag.prepare_train_batch(L, Rt, kn, base, size, first, disp_gt_raw=raw)
    torch.cuda.current_stream().wait_stream(side)
    first.refill(second)
    graph.replay()
    torch.cuda.synchronize()
    assert set(batch) == set(want)
    for k in want:
        assert same_bits(batch[k], want[k]), k
    for s in "lr":
        keep = torch.from_numpy(~R.rect_mask(second.rects[1][0] if s == "r" else [], size))
        assert same_bits(batch[("color_aug", 0, s)].cpu()[0][:, keep], torch.from_numpy(g["aug_" + s])[0][:, keep]), s


def test_a_launch_plan_replays_the_training_batch():
    g, L, Rt, kn, raw, base = _train_inputs()
    size = tuple(int(v) for v in g["size"])
    aug = fixture_aug(g)
    with _lib.Recorder() as rec:
        fr = ag.augment_frames(L, Rt, aug, size)
        disp = ag.disp_window_from_uint16(raw, aug, size)
    assert [n for n, _ in rec.log] == ["ts_frames_augment_fwd", "ts_disp_u16_window_fwd"]
    want = {k: v.clone() for k, v in fr.items()}
    want_disp = disp.clone()
    for t in list(fr.values()) + [disp]:
        t.fill_(float("nan"))
    rec.run()
    torch.cuda.synchronize()
    for k in want:
        assert same_bits(fr[k], want[k]), k
    assert same_bits(disp, want_disp)


def test_device_side_values_are_clamped():
    """what is already in the device table cannot be refused: an origin outside the frame is clamped, a rectangle is clipped"""
    g = load("augment_identity")
    size = tuple(int(v) for v in g["size"])
    H, W = size
    L, Rt = gpu(g["left"]), gpu(g["right"])
    Hs, Ws = g["left"].shape[1:3]
    aug = ag.Augmentation.identity(2, crop=[(0, 0), (0, 0)], device=_dev())
    t = aug.table_host()
    t[:, 0, 6:8] = (-5, 1000)
    t[:, 1, 6:8] = (1000, -7)
    t[1, 0, 8] = 1
    t[1, 0, 9:13] = (-3, W - 4, 10, 50)                                               # leaves the window at the top right
    aug.table.copy_(torch.from_numpy(t))
    got = ag.augment_frames(L, Rt, aug, size)
    want = pp.prepare_frames(L, Rt, size=size, crop=[(0, Ws - W), (Hs - H, 0)])
    for k in ("color_l", "color_r", "color_aug_l"):
        assert same_bits(got[k], want[k]), k
    inside = torch.from_numpy(R.rect_mask([(0, W - 4, 7, 4)], size)).to(_dev())
    assert same_bits(got["color_aug_r"][1], want["color_aug_r"][1])
    assert same_bits(got["color_aug_r"][0][:, ~inside], want["color_aug_r"][0][:, ~inside])
    assert (got["color_aug_r"][0][:, inside] != want["color_aug_r"][0][:, inside]).float().mean() > 0.99


def test_refusals():
    dev = _dev()
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8, device=dev)
    ident = lambda B, **k: ag.Augmentation.identity(B, device=dev, **k)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ag.augment_frames(torch.zeros(8, 8, 3, dtype=torch.uint8), None, ident(1), (8, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ag.augment_frames(u8(8, 8, 3), None, ag.Augmentation.identity(1).to("cpu"), (8, 8))
    with pytest.raises(TypeError, match=r"uint8.*\(8, 8, 3\)"):
        ag.augment_frames(torch.zeros(8, 8, 3, device=dev), None, ident(1), (8, 8))
    with pytest.raises(ValueError, match=r"three channels.*\(2, 8, 8, 4\)"):
        ag.augment_frames(u8(2, 8, 8, 4), None, ident(2), (8, 8))
    with pytest.raises(ValueError, match="layout must be"):
        ag.augment_frames(u8(8, 8, 3), None, ident(1), (8, 8), layout="NHWC")
    with pytest.raises(ValueError, match=r"\(8, 8\) cannot be cropped to \(9, 8\)"):
        ag.augment_frames(u8(8, 8, 3), None, ident(1), (9, 8))
    with pytest.raises(ValueError, match=r"2 eye\(s\) x 3 image\(s\), the frames are 2 x 2"):
        ag.augment_frames(u8(2, 8, 8, 3), u8(2, 8, 8, 3), ident(3), (8, 8))
    with pytest.raises(ValueError, match=r"1 eye\(s\) x 2 image\(s\), the frames are 2 x 2"):
        ag.augment_frames(u8(2, 8, 8, 3), u8(2, 8, 8, 3), ident(2, eyes=1), (8, 8))
    with pytest.raises(TypeError, match="must be an Augmentation"):
        ag.augment_frames(u8(8, 8, 3), None, torch.zeros(1, 1, 96, dtype=torch.int32, device=dev), (8, 8))
    with pytest.raises(ValueError, match=r"crop origin \(3, 0\).*\(6, 8\).*\(8, 8\)"):
        ag.augment_frames(u8(8, 8, 3), None, ident(1, crop=[(3, 0)], eyes=1), (6, 8))
    with pytest.raises(ValueError, match=r"rectangle \(0, 0, 7, 8\).*\(6, 8\) window"):
        ag.augment_frames(u8(8, 8, 3), u8(8, 8, 3), ag.Augmentation.from_values([[{}], [dict(rects=[(0, 0, 7, 8)])]], device=dev), (6, 8))
    with pytest.raises(TypeError, match="out must be fp32"):
        ag.augment_frames(u8(8, 8, 3), None, ident(1), (8, 8), out=torch.zeros(1, 3, 8, 8, dtype=torch.float64, device=dev))
    with pytest.raises(ValueError, match="2 out tensors for 1 eyes"):
        ag.augment_frames(u8(8, 8, 3), None, ident(1), (8, 8), out=(torch.zeros(1, 3, 8, 8, device=dev),) * 2)
    with pytest.raises(ValueError, match="a stereo pair"):
        ag.prepare_train_batch(u8(8, 8, 3), None, torch.eye(4, device=dev), 0.5, (8, 8), ident(1))
    with pytest.raises(TypeError, match="raw must be uint16"):
        ag.disp_window_from_uint16(torch.zeros(8, 8, device=dev), ident(1), (4, 4))
    with pytest.raises(ValueError, match=r"\(8, 8\) cannot be cropped to \(4, 9\)"):
        ag.disp_window_from_uint16(torch.zeros(8, 8, dtype=torch.int16, device=dev), ident(1), (4, 9))
