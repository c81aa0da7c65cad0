"""Input preparation on the device (temporalstereo_amd/preprocess.py, csrc/preprocess.hip) against the reference's own runs recorded
in tests/golden/prepare_*.npz (tools/gen_golden.py --only-prepare: StereoDatasetBase.__getitem__ / do_transform, read_image,
read_disparity).

Bars, none taken from the code under test:
  - everything without taps is compared with torch.equal: `color` in every case, `color_aug` of the same-size and crop cases, the
    decoded 16-bit map and its mask.  Each value is a single correctly rounded IEEE operation chain in the reference's order.
  - a resized `color_aug` has two bars per case, both from recorded reference runs: max |device - reference fp32| <= dev32_64 and
    max |device - reference fp64| <= 1.5 x dev32_64, dev32_64 = max |reference fp32 - reference fp64| of that case (the bar of
    tests/test_fullsize_gpu.py: no further from the fp64 answer than 1.5 x the reference's own fp32 run).
  - K: 1 ulp (2^-23 relative) on the entries that are non-zero in the closed form, 1e-12 absolute on its structural zeros;
    K @ inv_K within 1e-6 of the identity.
"""
import os

import numpy as np
import pytest
import torch

from compare import dev as _dev, gpu
from temporalstereo_amd import _lib, preprocess as pp

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EXACT = ("prepare_same", "prepare_ramp", "prepare_train_crop")
RESIZED = ("prepare_dataset_up", "prepare_video_up", "prepare_down", "prepare_degenerate")
WITH_K = ("prepare_same", "prepare_dataset_up", "prepare_video_up", "prepare_down", "prepare_train_crop")


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def run_case(g, k, **kw):
    L, R = gpu(g["left%d" % k]), gpu(g["right%d" % k])
    size = tuple(g["aug_l%d" % k].shape[-2:])
    crop = [tuple(c) for c in g["crop%d" % k].tolist()] if "crop%d" % k in g else None
    return pp.prepare_frames(L, R, size=size, crop=crop, **kw)


@pytest.mark.parametrize("name", EXACT + RESIZED)
def test_color_equals_the_reference(name):
    g = load(name)
    for k in range(int(g["subs"])):
        r = run_case(g, k)
        for s in "lr":
            assert torch.equal(r["color_" + s].cpu(), torch.from_numpy(g["color_%s%d" % (s, k)])), (name, k, s)


@pytest.mark.parametrize("name", EXACT)
def test_color_aug_without_taps_equals_the_reference(name):
    g = load(name)
    for k in range(int(g["subs"])):
        r = run_case(g, k)
        for s in "lr":
            got, want = r["color_aug_" + s].cpu(), torch.from_numpy(g["aug_%s%d" % (s, k)])
            assert torch.equal(got, want), (name, k, s, float((got - want).abs().max()))


@pytest.mark.parametrize("name", RESIZED)
def test_resized_color_aug_within_the_reference_s_own_error(name):
    g = load(name)
    dev32_64 = float(g["dev32_64"])
    for k in range(int(g["subs"])):
        r = run_case(g, k)
        for s in "lr":
            got = r["color_aug_" + s].cpu().numpy().astype(np.float64)
            ref32 = g["aug_%s%d" % (s, k)].astype(np.float64)
            ref64 = ref32 + g["d64_%s%d" % (s, k)].astype(np.float64)
            assert got.shape == ref32.shape
            d32, d64 = float(np.abs(got - ref32).max()), float(np.abs(got - ref64).max())
            print("%s sub %d %s: max |device - ref fp32| %.3g (bar %.3g), max |device - ref fp64| %.3g (bar %.3g)"
                  % (name, k, s, d32, dev32_64, d64, 1.5 * dev32_64))
            assert d32 <= dev32_64, (name, k, s, d32, dev32_64)
            assert d64 <= 1.5 * dev32_64, (name, k, s, d64, dev32_64)


@pytest.mark.parametrize("name", WITH_K)
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_intrinsics_pyramid(name, dtype):
    g = load(name)
    want_K, want_inv = g["K0"].astype(np.float64), g["inv_K0"].astype(np.float64)
    S = want_K.shape[1]
    kn = gpu(g["K_norm0"]).to(dtype)
    K, inv = pp.intrinsics_pyramid(kn, tuple(int(v) for v in g["k_size0"]), S)
    assert K.shape == (S, 4, 4) and K.dtype == torch.float32
    K, inv = K.cpu().numpy().astype(np.float64), inv.cpu().numpy().astype(np.float64)
    # fp32 intrinsics carry their own rounding (2^-24 relative) into both results: the bar is stated for the fp64 form the
    # reference uses; the fp32 form is held to the rounding of its input on top (3 ulp)
    ulp = 2.0 ** -23 * (1 if dtype == torch.float64 else 3)
    closed_form_zero = np.ones((4, 4), dtype=bool)
    closed_form_zero[[0, 1, 2, 3], [0, 1, 2, 3]] = False
    closed_form_zero[0, 2] = closed_form_zero[1, 2] = False
    for b in range(want_K.shape[0]):
        for s in range(S):
            for got, want in ((K[s], want_K[b, s]), (inv[s], want_inv[b, s])):
                nz = ~closed_form_zero
                assert np.all(np.abs(got[nz] - want[nz]) <= ulp * np.abs(want[nz])), (name, s, got, want)
                assert np.abs(got[closed_form_zero] - want[closed_form_zero]).max() <= 1e-12, (name, s)
            assert np.abs(K[s] @ inv[s] - np.eye(4)).max() <= 1e-6
    # a batch of matrices equals the single ones
    Kb, invb = pp.intrinsics_pyramid(torch.stack([kn, kn * 1.0]), tuple(int(v) for v in g["k_size0"]), S)
    assert Kb.shape == (2, S, 4, 4) and np.array_equal(Kb[1].cpu().numpy(), K.astype(np.float32)) and np.array_equal(invb[0].cpu().numpy(), inv.astype(np.float32))


def test_default_num_scales_is_the_reference_s():
    g = load("prepare_dataset_up")
    K, _ = pp.intrinsics_pyramid(gpu(g["K_norm0"]), tuple(int(v) for v in g["k_size0"]))
    assert K.shape[0] == g["K0"].shape[1]


def test_disp_from_uint16():
    g = load("prepare_disp16")
    raw = g["raw0"]
    want, want_valid = torch.from_numpy(g["disp0"]), torch.from_numpy(g["valid0"])
    forms = [torch.from_numpy(raw.view(np.int16)).to(_dev()), torch.from_numpy(raw.astype(np.int32)).to(_dev())]
    if hasattr(torch, "uint16"):
        forms.append(torch.from_numpy(raw).to(_dev()))
    for r in forms:
        d, v = pp.disp_from_uint16(r, with_valid=True)
        assert d.shape == (1, 1) + raw.shape[1:] and v.dtype == torch.bool
        assert torch.equal(d.cpu(), want) and torch.equal(v.cpu(), want_valid), r.dtype
        assert torch.equal(pp.disp_from_uint16(r[0]).cpu(), want[0, 0])                   # one map, and without the mask
    # ragged tails and unaligned starts: every prefix length mod 4, from an odd element on
    flat = forms[0].reshape(-1)
    for off, n in ((1, 61), (3, 62), (2, 63), (1, 64)):
        d, v = pp.disp_from_uint16(flat[off:off + n].reshape(1, n), with_valid=True)
        assert torch.equal(d.cpu().reshape(-1), want.reshape(-1)[off:off + n]) and torch.equal(v.cpu().reshape(-1), want_valid.reshape(-1)[off:off + n])
    assert torch.equal(pp.disp_from_uint16(forms[0], scale=128.0).cpu(), want * 2)


def test_one_launch_writes_both_eyes_and_layouts_agree():
    for name in ("prepare_train_crop", "prepare_dataset_up", "prepare_same"):
        g = load(name)
        both = run_case(g, 0)
        L, R = gpu(g["left0"]), gpu(g["right0"])
        size = tuple(g["aug_l0"].shape[-2:])
        crop = [tuple(c) for c in g["crop0"].tolist()] if "crop0" in g else None
        alone = pp.prepare_frames(L, size=size, crop=crop)
        assert set(alone) == {"color_l", "color_aug_l"}
        assert torch.equal(alone["color_l"], both["color_l"]) and torch.equal(alone["color_aug_l"], both["color_aug_l"])
        chw = pp.prepare_frames(L.permute(0, 3, 1, 2).contiguous(), R.permute(0, 3, 1, 2).contiguous(), size=size, crop=crop, layout='CHW')
        for k in both:
            assert torch.equal(chw[k], both[k]), (name, k)
        one = pp.prepare_frames(L[1] if L.shape[0] > 1 else L[0], size=size, crop=None if crop is None else crop[1], color=False)
        assert set(one) == {"color_aug_l"} and torch.equal(one["color_aug_l"], both["color_aug_l"][1 if L.shape[0] > 1 else 0])
        if crop is not None:
            as_tensor = pp.prepare_frames(L, R, size=size, crop=torch.tensor(crop, dtype=torch.int32, device=_dev()))
            for k in both:
                assert torch.equal(as_tensor[k], both[k]), (name, k)
            # a device tensor cannot be refused without a synchronisation: its origins are clamped into the image
            Hs, Ws = L.shape[1:3]
            wild = torch.tensor([[-7, -1], [10 ** 6, 10 ** 6]], dtype=torch.int32, device=_dev())
            clamped = pp.prepare_frames(L, R, size=size, crop=wild)
            inside = pp.prepare_frames(L, R, size=size, crop=[(0, 0), (Hs - size[0], Ws - size[1])])
            for k in both:
                assert torch.equal(clamped[k], inside[k]), (name, k)


@pytest.mark.parametrize("name", ["prepare_same", "prepare_dataset_up", "prepare_train_crop", "prepare_ramp"])
def test_out_slices_of_a_larger_buffer_stay_inside_their_images(name):
    g = load(name)
    want = run_case(g, 0)
    B, _, H, W = want["color_aug_l"].shape
    poison = float("nan")
    # images inside a flat pool, 12 bytes in, at a batch stride of two images and five floats: rows start on every alignment
    n = 3 * H * W
    stride = 2 * n + 5
    pool = [torch.full((B * stride + 7,), poison, device=_dev()) for _ in range(2)]
    outs = tuple(torch.as_strided(pool[e], (B, 3, H, W), (stride, H * W, W, 1), 3) for e in range(2))
    crop = [tuple(c) for c in g["crop0"].tolist()] if "crop0" in g else None
    r = pp.prepare_frames(gpu(g["left0"]), gpu(g["right0"]), size=(H, W), crop=crop, color=False, out=outs)
    assert r["color_aug_l"].data_ptr() == outs[0].data_ptr() and r["color_aug_r"].data_ptr() == outs[1].data_ptr()
    for e, s in enumerate("lr"):
        assert torch.equal(outs[e], want["color_aug_" + s])
        written = torch.zeros_like(pool[e], dtype=torch.bool)
        torch.as_strided(written, (B, 3, H, W), (stride, H * W, W, 1), 3).fill_(True)
        assert bool(torch.isnan(pool[e][~written]).all()) and not bool(torch.isnan(pool[e][written]).any())


def test_prepare_batch_is_the_reference_s_dictionary():
    g = load("prepare_video_up")
    size = tuple(g["aug_l0"].shape[-2:])
    d16 = load("prepare_disp16")
    batch = pp.prepare_batch(gpu(g["left0"]), gpu(g["right0"]), gpu(g["K_norm0"]), float(g["baseline0"]), size, timestamp=0,
                             disp_gt_raw=gpu(d16["raw0"].view(np.int16)), num_scales=1)
    assert set(batch) == {("color", 0, "l"), ("color", 0, "r"), ("color_aug", 0, "l"), ("color_aug", 0, "r"), ("K", 0), ("inv_K", 0),
                          "baseline", ("disp_gt", 0, "l")}
    for s in "lr":
        assert torch.equal(batch[("color", 0, s)].cpu(), torch.from_numpy(g["color_%s0" % s]))
        assert float((batch[("color_aug", 0, s)].cpu() - torch.from_numpy(g["aug_%s0" % s])).abs().max()) <= float(g["dev32_64"])
    assert batch[("K", 0)].shape == (1, 4, 4) and torch.equal(batch[("K", 0)].cpu(), torch.from_numpy(g["K0"][:, 0]))
    assert np.abs(batch[("inv_K", 0)].cpu().numpy() - g["inv_K0"][:, 0]).max() <= 2.0 ** -23 * np.abs(g["inv_K0"]).max()
    assert batch["baseline"].shape == (1, 1, 1, 1) and float(batch["baseline"]) == float(g["baseline0"])
    assert torch.equal(batch[("disp_gt", 0, "l")].cpu(), torch.from_numpy(d16["disp0"]))
    # the training form: crop, K at the un-cropped resolution, the dataset's number of scales
    g = load("prepare_train_crop")
    size = tuple(g["aug_l0"].shape[-2:])
    batch = pp.prepare_batch(gpu(g["left0"]), gpu(g["right0"]), gpu(g["K_norm0"]), 1.0, size, timestamp=3,
                             crop=[tuple(c) for c in g["crop0"].tolist()], k_size=tuple(int(v) for v in g["k_size0"]))
    S = g["K0"].shape[1]
    assert ("K", S - 1) in batch and ("K", S) not in batch
    for s in range(S):
        assert torch.equal(batch[("K", s)].cpu(), torch.from_numpy(g["K0"][:, s]))
    for s in "lr":
        assert torch.equal(batch[("color", 3, s)].cpu(), torch.from_numpy(g["color_%s0" % s]))
        assert torch.equal(batch[("color_aug", 3, s)].cpu(), torch.from_numpy(g["aug_%s0" % s]))


def test_prepared_frames_drive_the_bound_engine():
    """uint8 frames -> prepare_frames(out=the engine's bound image tensors) -> the same disparity, bit for bit, as the same images
    normalised on the host and uploaded (same bytes in, same plan)."""
    import synth
    from helpers import load as load_golden, dims_from_golden, aggregator_inputs
    from test_aggregator_gpu import _build
    from temporalstereo_amd.aggregation.engine import InferenceEngine
    g = load_golden("agg_tiny_single")
    dev = _dev()
    dims = dims_from_golden(g)
    net = _build(dims, int(g["seed"]), dev, golden=g)
    lf, rf, il, ir, prev = aggregator_inputs(g, dims, dev)
    B, _, H, W = il.shape
    u8 = [synth._rs(synth.SEED0 + 950, tag).randint(0, 256, size=(B, H, W, 3)).astype(np.uint8) for tag in ("engL", "engR")]
    mean, std = torch.tensor(pp.IMAGENET_MEAN), torch.tensor(pp.IMAGENET_STD)
    host = [((torch.from_numpy(a).permute(0, 3, 1, 2).contiguous().to(torch.float32).div(255) - mean[:, None, None]) / std[:, None, None])
            for a in u8]
    eng = InferenceEngine(net, backend="native", replay="plan", inputs="bind")
    il.copy_(host[0].to(dev)); ir.copy_(host[1].to(dev))
    torch.cuda.synchronize()
    want = [x.clone() for x in eng(lf, rf, il, ir, dict(prev))[0]]
    il.zero_(); ir.zero_()
    torch.cuda.synchronize()
    other = [x.clone() for x in eng(lf, rf, il, ir, dict(prev))[0]]
    assert float((other[0] - want[0]).abs().max()) > 1e-3                    # the images matter to the result
    r = pp.prepare_frames(gpu(u8[0]), gpu(u8[1]), color=False, out=(il, ir))
    assert r["color_aug_l"] is il and r["color_aug_r"] is ir
    torch.cuda.synchronize()
    got = eng(lf, rf, il, ir, dict(prev))[0]
    torch.cuda.synchronize()
    assert len(eng._graphs) == 1
    assert torch.equal(il.cpu(), host[0]) and torch.equal(ir.cpu(), host[1])
    for a, b in zip(got, want):
        assert torch.equal(a, b)


def test_no_host_synchronisation_graph_capture_and_replay():
    """prepare_batch inside a stream capture on a side stream (a synchronisation or a host read of device data makes the capture
    raise), then one replay on new bytes copied into the captured input buffers."""
    g, d16 = load("prepare_dataset_up"), load("prepare_disp16")
    size = tuple(g["aug_l0"].shape[-2:])
    B = g["left0"].shape[0]
    L, R, kn = gpu(g["left0"]), gpu(g["right0"]), gpu(g["K_norm0"])
    raw = gpu(np.repeat(d16["raw0"].view(np.int16), B, axis=0))
    base = torch.full((B,), 0.54, device=_dev())
    crop = torch.zeros((B, 2), dtype=torch.int32, device=_dev())
    want = pp.prepare_batch(L.flip(1).contiguous(), R.flip(2).contiguous(), kn, base, size, disp_gt_raw=raw)
    want_crop = pp.prepare_frames(L.flip(1).contiguous(), size=(8, 12), crop=torch.tensor([[3, 5], [1, 2]], dtype=torch.int32, device=_dev()))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            batch = pp.prepare_batch(L, R, kn, base, size, disp_gt_raw=raw)
            cropped = pp.prepare_frames(L, size=(8, 12), crop=crop)
    torch.cuda.current_stream().wait_stream(side)
    L.copy_(L.flip(1).contiguous()); R.copy_(R.flip(2).contiguous())
    crop.copy_(torch.tensor([[3, 5], [1, 2]], dtype=torch.int32, device=_dev()))
    graph.replay()
    torch.cuda.synchronize()
    assert set(batch) == set(want)
    for k in want:
        assert torch.equal(batch[k], want[k]), k
    for k in want_crop:
        assert torch.equal(cropped[k], want_crop[k]), k


def test_a_launch_plan_replays_the_three_entries():
    g, d16 = load("prepare_down"), load("prepare_disp16")
    size = tuple(g["aug_l0"].shape[-2:])
    L, R, kn, raw = gpu(g["left0"]), gpu(g["right0"]), gpu(g["K_norm0"]), gpu(d16["raw0"].view(np.int16))
    with _lib.Recorder() as rec:
        fr = pp.prepare_frames(L, R, size=size)
        K, inv = pp.intrinsics_pyramid(kn, size, 1)
        disp = pp.disp_from_uint16(raw)
    assert [n for n, _ in rec.log] == ["ts_frames_prepare_fwd", "ts_intrinsics_pyramid_fwd", "ts_disp_u16_decode_fwd"]
    want = {k: v.clone() for k, v in fr.items()}
    want_K, want_disp = K.clone(), disp.clone()
    for t in list(fr.values()) + [K, inv, disp]:
        t.fill_(float("nan"))
    rec.run()
    torch.cuda.synchronize()
    for k in want:
        assert torch.equal(fr[k], want[k]), k
    assert torch.equal(K, want_K) and torch.equal(disp, want_disp) and not bool(torch.isnan(inv).any())


def test_refusals():
    dev = _dev()
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pp.prepare_frames(torch.zeros(8, 8, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pp.prepare_frames(u8(8, 8, 3), torch.zeros(8, 8, 3, dtype=torch.uint8))
    with pytest.raises(TypeError, match=r"uint8.*\(8, 8, 3\)"):
        pp.prepare_frames(torch.zeros(8, 8, 3, device=dev))
    with pytest.raises(ValueError, match=r"three channels.*\(2, 8, 8, 4\)"):
        pp.prepare_frames(u8(2, 8, 8, 4))
    with pytest.raises(ValueError, match=r"\(8, 8\) cannot be cropped to \(9, 8\)"):
        pp.prepare_frames(u8(8, 8, 3), size=(9, 8), crop=(0, 0))
    with pytest.raises(ValueError, match=r"crop origin \(3, 0\).*\(6, 8\).*\(8, 8\)"):
        pp.prepare_frames(u8(8, 8, 3), size=(6, 8), crop=(3, 0))
    with pytest.raises(ValueError, match=r"crop origin \(0, -1\)"):
        pp.prepare_frames(u8(2, 8, 8, 3), size=(6, 6), crop=[(0, 0), (0, -1)])
    with pytest.raises(ValueError, match="one \\(ch, cw\\) per image"):
        pp.prepare_frames(u8(3, 8, 8, 3), size=(6, 6), crop=[(0, 0), (1, 1)])
    with pytest.raises(ValueError, match=r"crop tensor is int32 \[2,2\]"):
        pp.prepare_frames(u8(2, 8, 8, 3), size=(6, 6), crop=torch.zeros(2, 2, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError, match="window's size"):
        pp.prepare_frames(u8(8, 8, 3), crop=(0, 0))
    with pytest.raises(ValueError, match=r"empty batch.*\(0, 8, 8, 3\)"):
        pp.prepare_frames(u8(0, 8, 8, 3))
    with pytest.raises(ValueError, match=r"left has shape \(8, 8, 3\), right \(8, 9, 3\)"):
        pp.prepare_frames(u8(8, 8, 3), u8(8, 9, 3))
    with pytest.raises(ValueError, match=r"out has shape \(1, 3, 8, 9\), \(1, 3, 8, 8\) expected"):
        pp.prepare_frames(u8(8, 8, 3), out=torch.zeros(1, 3, 8, 9, device=dev))
    with pytest.raises(ValueError, match="dense"):
        pp.prepare_frames(u8(8, 8, 3), out=torch.zeros(1, 3, 8, 16, device=dev)[..., ::2])
    with pytest.raises(ValueError, match=r"K_norm.*\(3, 3\)"):
        pp.intrinsics_pyramid(torch.eye(3, device=dev), (8, 8))
    with pytest.raises(TypeError, match="fp32 or fp64"):
        pp.intrinsics_pyramid(torch.eye(4, device=dev).half(), (8, 8))
    with pytest.raises(ValueError, match="5 scales of a 8x8"):
        pp.intrinsics_pyramid(torch.eye(4, device=dev), (8, 8), 5)
    with pytest.raises(TypeError, match=r"uint16.*float32.*\(4, 4\)"):
        pp.disp_from_uint16(torch.zeros(4, 4, device=dev))
    with pytest.raises(ValueError, match=r"\(2, 2, 4, 4\)"):
        pp.disp_from_uint16(torch.zeros(2, 2, 4, 4, dtype=torch.int16, device=dev))
    with pytest.raises(ValueError, match="stereo pair"):
        pp.prepare_batch(u8(8, 8, 3), None, torch.eye(4, device=dev), 1.0, (8, 8))
    # over the C ABI: the error status and the thread's message
    L = _lib.lib()
    x = u8(8, 8, 3)
    o = torch.zeros(1, 3, 8, 8, device=dev)
    m, s = pp.IMAGENET_MEAN, pp.IMAGENET_STD
    assert L.ts_frames_prepare_fwd(None, None, 1, 8, 8, 0, *m, *s, 8, 8, None, None, None, 0, o.data_ptr(), None, 192, None) == -1
    assert b"NULL" in L.ts_last_error_string()
    assert L.ts_frames_prepare_fwd(x.data_ptr(), None, 0, 8, 8, 0, *m, *s, 8, 8, None, None, None, 0, o.data_ptr(), None, 192, None) == -2
    assert b"bad size" in L.ts_last_error_string()
    assert L.ts_frames_prepare_fwd(x.data_ptr(), None, 1, 8, 8, 0, *m, *s, 8, 8, None, None, None, 0, o.data_ptr() + 2, None, 192, None) == -4
    torch.cuda.synchronize()
    assert float(o.abs().max()) == 0.0                                       # nothing was launched
