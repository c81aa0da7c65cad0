"""Colour maps and the 16-bit map on the device (temporalstereo_amd/visualization.py, csrc/render.hip) against the reference's own
disp_to_color / disp_err_to_color / disp_err_to_colorbar (tests/golden/render_*.npz, tools/gen_golden.py --only-render).

How results are compared:
  continuous outputs (disp_to_color)   |device - reference| <= 5e-6 * max(1, |reference|) on every component (the ramp's largest
                                       slope is 1 / 0.114 = 8.78 per unit of t = d / max, and t is one fp32 division on both sides);
                                       where the estimate is rescaled, plus 8.78 / max * 4 * the recorded fp32-vs-fp64 deviation of
                                       the reference's rescaled map.  NaN where the reference's is NaN.
  discontinuous outputs                exact outside the fixture's near-tie mask (computed by the generator from the reference
                                       alone, at most 1 % / 8 % of a case), the adjacent class / index / code accepted inside it.
  statistics                           exact on same-size inputs; within 4 x the recorded deviation (counts: within the number of
                                       pixels that close to a range bound) where the estimate is rescaled.
"""
import os

import numpy as np
import pytest
import torch

import synth
from temporalstereo_amd import _lib, visualization as vz
from temporalstereo_amd.losses import rescale_to_full

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ("render_dense", "render_sparse", "render_rescaled", "render_empty_range", "render_small_errors", "render_given_max",
         "render_batch3", "render_nonfinite")
DEV = torch.device("cuda:0")
TABLES = dict(np.load(os.path.join(GOLDEN, "render_tables.npz")))
JET32 = TABLES["jet"].astype(np.float32)
CLASS32 = TABLES["class_rgb"].astype(np.float32)


def _load(name):
    g = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    est = torch.from_numpy(g["est"]).to(DEV)
    gt = torch.from_numpy(g["gt"]).to(DEV)
    H, W = gt.shape[-2:]
    full = est if est.shape[-2:] == gt.shape[-2:] else rescale_to_full(est, (H, W))
    return g, est, gt, full


def _np(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16) if t.dtype == torch.uint16 else t.cpu().numpy()


def _same(a, b):
    """Bit-identical tensors (NaN included)."""
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape, a.dtype, b.dtype)
    bits = {torch.float32: torch.int32, torch.uint16: torch.int16}.get(a.dtype, a.dtype)
    return torch.equal(a.contiguous().view(bits), b.contiguous().view(bits))


def _check_continuous(got, ref, extra, what):
    got, ref = got.astype(np.float64), ref.astype(np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "%s: NaN pattern differs at %d components" % (what, (np.isnan(got) != np.isnan(ref)).sum())
    ok = ~np.isnan(ref)
    err = np.abs(got[ok] - ref[ok])
    bound = 5e-6 * np.maximum(1.0, np.abs(ref[ok])) + extra
    worst = float((err / bound).max()) if err.size else 0.0
    print("%s: largest |device - reference| %.3g, largest error / bound %.3g" % (what, err.max() if err.size else 0.0, worst))
    assert worst <= 1.0, what


def _check_indexed(got, idx, tie, table, lo, hi, what):
    """got [...,3] fp32 colours; idx the reference's table index per pixel (outside lo..hi: black); inside `tie` the adjacent
    index is accepted too."""
    def colour(i):
        return np.where(((i >= lo) & (i <= hi))[..., None], table[np.clip(i, lo, hi)], np.float32(0))
    idx = idx.astype(np.int64)
    exact = np.all(got == colour(idx), axis=-1)
    inside = (idx >= lo) & (idx <= hi)
    near = np.all(got == colour(idx - 1), axis=-1) | np.all(got == colour(idx + 1), axis=-1)
    print("%s: %d of %d pixels differ from the reference's index, %d of them inside the near-tie set of %d"
          % (what, (~exact).sum(), exact.size, (~exact & tie).sum(), tie.sum()))
    assert np.all(exact | (tie & inside & near)), "%s: %d pixels wrong outside the near-tie set" % (what, (~(exact | (tie & inside & near))).sum())


def _check_codes(got, ref, tie, what):
    got, ref = got.astype(np.int64), ref.astype(np.int64)
    d = np.abs(got - ref)
    print("%s: %d of %d codes differ, %d of them inside the near-tie set of %d" % (what, (d > 0).sum(), d.size, ((d > 0) & tie).sum(), tie.sum()))
    assert np.all((d == 0) | (tie & (d == 1))), "%s: %d codes wrong outside the near-tie set" % (what, (~((d == 0) | (tie & (d == 1)))).sum())


def _u8(ref):
    """floor(255 v + 0.5) of a reference colour array after the clamp to [0,1], NaN -> 0."""
    v = np.clip(np.nan_to_num(ref.astype(np.float64), nan=0.0), 0.0, 1.0)
    return np.floor(255.0 * v + 0.5).astype(np.int64)


def _extra(g):
    """The rescaled case's allowance on a colour component: 8.78 / max * 4 * the recorded deviation of the rescaled map."""
    if str(g["group"]) != "rescaled":
        return 0.0
    return 8.78 / float(g["stats"][:, 2].min()) * 4.0 * float(g["rescale_dev"])


@pytest.mark.parametrize("name", CASES)
def test_disp_to_color_against_reference(name):
    g, est, gt, full = _load(name)
    if int(g["has_max"]):
        got = vz.disp_to_color(full, float(g["max_disp"]))
        _check_continuous(_np(got), g["disp_color"], 0.0, name + " disp_to_color(max_disp)")
        got_t = vz.disp_to_color(full, torch.full((full.shape[0],), float(g["max_disp"]), device=DEV))
        assert _same(got, got_t)
        got8 = vz.disp_to_color(full, float(g["max_disp"]), dtype=torch.uint8)
        _check_codes(_np(got8), _u8(g["disp_color"]), g["disp_color_u8_tie"], name + " disp_to_color uint8")
        clipped = vz.disp_to_color(full, float(g["max_disp"]), clip=True)
        _check_continuous(_np(clipped), np.clip(g["disp_color"], 0, 1), 0.0, name + " disp_to_color(clip)")
        assert (g["disp_color"] > 1).any() and (g["disp_color"] < 0).any() and float(got.max()) > 1 and float(got.min()) < 0
        return
    cat = torch.cat((full, gt), dim=-2)
    got = vz.disp_to_color(cat)
    assert got.shape == (cat.shape[0], cat.shape[2], cat.shape[3], 3) and got.dtype == torch.float32 and got.is_cuda
    _check_continuous(_np(got), g["cat_color"], _extra(g), name + " disp_to_color(cat(est, gt))")
    got8 = vz.disp_to_color(cat, dtype=torch.uint8)
    _check_codes(_np(got8), _u8(g["cat_color"]), g["cat_color_u8_tie"], name + " disp_to_color uint8")
    # a single [H,W] map, as the reference takes it
    one = vz.disp_to_color(cat[0, 0])
    assert one.shape == got.shape[1:] and _same(one, got[0])


@pytest.mark.parametrize("name", CASES)
def test_error_maps_and_uint16_against_reference(name):
    g, est, gt, full = _load(name)
    cls = vz.disp_err_to_color(full, gt)
    _check_indexed(_np(cls), g["class_idx"], g["class_tie"], CLASS32, 0, 9, name + " disp_err_to_color")
    bar = vz.disp_err_to_colorbar(full, gt, with_bar=True, cmap='jet')
    H = gt.shape[-2]
    assert bar.shape == (gt.shape[0], H + 50, gt.shape[-1], 3)
    _check_indexed(_np(bar)[:, :H], g["jet_idx"], g["jet_tie"], JET32, 0, 255, name + " disp_err_to_colorbar")
    legend = np.broadcast_to(JET32[g["bar_idx"]], (gt.shape[0], 50, gt.shape[-1], 3))
    assert np.array_equal(_np(bar)[:, H:], legend), name + " legend"
    assert _same(vz.disp_err_to_colorbar(full, gt), bar[:, :H].contiguous())
    u16 = vz.disp_to_uint16(full)
    assert u16.dtype == torch.uint16 and u16.shape == (gt.shape[0], H, gt.shape[-1])
    _check_codes(_np(u16), g["u16"], g["u16_tie"], name + " disp_to_uint16")


@pytest.mark.parametrize("name", CASES)
def test_statistics_against_reference(name):
    g, est, gt, full = _load(name)
    st = vz.render_stats(est, gt)
    again = vz.render_stats(est, gt)
    assert _same(st, again), "statistics differ from run to run"
    got = _np(st).astype(np.float64)
    cnt = _np(vz.range_counts(st)).astype(np.int64)
    ref = g["stats"]
    vals = np.concatenate([got[:, 0:4], got[:, 8:14], got[:, 16:22]], axis=1)
    rvals = ref[:, :16]
    assert np.array_equal(np.isnan(vals), np.isnan(rvals)), (name, vals, rvals)
    if str(g["group"]) != "rescaled":
        assert np.array_equal(vals, rvals, equal_nan=True), (name, vals - rvals)
        assert np.array_equal(cnt, ref[:, 16:].astype(np.int64)), (name, cnt, ref[:, 16:])
    else:
        tol = 4.0 * float(g["rescale_dev"])
        fin = np.isfinite(rvals)
        print("%s: statistics off by at most %.3g (allowed %.3g); counts off by %s (allowed %s)"
              % (name, np.abs(vals[fin] - rvals[fin]).max(), tol, np.abs(cnt - ref[:, 16:]).tolist(), g["count_slack"].tolist()))
        assert np.array_equal(vals[~fin], rvals[~fin]) and np.all(np.abs(vals[fin] - rvals[fin]) <= tol)
        assert np.all(np.abs(cnt - ref[:, 16:].astype(np.int64)) <= g["count_slack"])


def _frame_by_drop_ins(full, gt, dtype, fmt, clip=True):
    return {'disp_color': vz.disp_to_color(torch.cat((full, gt), dim=-2), clip=clip, dtype=dtype, format=fmt),
            'error_map': vz.disp_err_to_color(full, gt, dtype=dtype, format=fmt),
            'error_bar_map': vz.disp_err_to_colorbar(full, gt, with_bar=True, dtype=dtype, format=fmt),
            'disp_u16': vz.disp_to_uint16(full)}


@pytest.mark.parametrize("name", CASES)
def test_render_frame_equals_drop_ins_and_fixture(name):
    g, est, gt, full = _load(name)
    for dtype in (torch.float32, torch.uint8):
        for fmt in ('HWC', 'CHW'):
            fr = vz.render_frame(est, gt, dtype=dtype, format=fmt)
            ref = _frame_by_drop_ins(full, gt, dtype, fmt)
            assert list(fr) == list(vz.OUTPUTS)
            for k in vz.OUTPUTS:
                assert _same(fr[k], ref[k]), "%s %s %s %s: render_frame differs from the drop-in" % (name, k, dtype, fmt)
    f32 = vz.render_frame(est, gt, dtype=torch.float32)
    u8 = vz.render_frame(est, gt)
    chw = vz.render_frame(est, gt, dtype=torch.float32, format='CHW')
    for k in ('disp_color', 'error_map', 'error_bar_map'):
        assert u8[k].dtype == torch.uint8
        v = f32[k]
        want = torch.floor(torch.nan_to_num(v, nan=0.0).clamp(0, 1) * 255 + 0.5).to(torch.uint8)
        assert torch.equal(u8[k], want), "%s %s: uint8 is not floor(255 * fp32 + 0.5)" % (name, k)
        assert _same(chw[k], f32[k].permute(0, 3, 1, 2).contiguous()), "%s %s: CHW differs from HWC" % (name, k)
    assert _same(u8['disp_u16'], f32['disp_u16'])
    # and against the fixture
    H = gt.shape[-2]
    if not int(g["has_max"]):
        _check_continuous(_np(f32['disp_color']), np.clip(g["cat_color"], 0, 1), _extra(g), name + " render_frame disp_color")
    _check_indexed(_np(f32['error_map']), g["class_idx"], g["class_tie"], CLASS32, 0, 9, name + " render_frame error_map")
    _check_indexed(_np(f32['error_bar_map'])[:, :H], g["jet_idx"], g["jet_tie"], JET32, 0, 255, name + " render_frame error_bar_map")
    _check_codes(_np(f32['disp_u16']), g["u16"], g["u16_tie"], name + " render_frame disp_u16")
    # without a ground truth: the estimate alone, its own maximum
    alone = vz.render_frame(est, size=gt.shape[-2:], dtype=torch.float32)
    assert list(alone) == ['disp_color', 'disp_u16']
    assert _same(alone['disp_color'], vz.disp_to_color(full, clip=True)) and _same(alone['disp_u16'], f32['disp_u16'])


def test_batch_equals_single_calls_and_runs_repeat():
    g, est, gt, full = _load("render_batch3")
    a = vz.render_frame(est, gt, dtype=torch.float32)
    b = vz.render_frame(est, gt, dtype=torch.float32)
    for k in a:
        assert _same(a[k], b[k]), k + ": two calls differ"
    for i in range(est.shape[0]):
        one = vz.render_frame(est[i:i + 1], gt[i:i + 1], dtype=torch.float32)
        for k in a:
            assert _same(one[k], a[k][i:i + 1].contiguous()), "%s: image %d alone differs from the batch" % (k, i)
    per_image = torch.tensor([30.0, 60.0, 90.0], device=DEV)
    c = vz.disp_to_color(est, per_image)
    for i in range(3):
        assert _same(c[i], vz.disp_to_color(est[i, 0], float(per_image[i])))


def _ramp_restated(d, mx):
    """disp_map in plain torch (float64 after the fp32 division), for maps that need no fixture."""
    edges = torch.tensor([0.0, 0.114, 0.299, 0.413, 0.587, 0.701, 0.886], dtype=torch.float64)
    width = torch.tensor([114.0, 185.0, 114.0, 174.0, 114.0, 185.0, 114.0], dtype=torch.float64) / 1000.0
    rows = torch.tensor([[0, 0, 0], [0, 0, 1], [1, 0, 0], [1, 0, 1], [0, 1, 0], [0, 1, 1], [1, 1, 0], [1, 1, 1]], dtype=torch.float64)
    t = (d / mx).double()
    s = (t.unsqueeze(-1) > edges[1:]).sum(-1)
    r = ((t - edges[s]) * (1.0 / width)[s]).unsqueeze(-1)
    return rows[s] * (1 - r) + rows[s + 1] * r


@pytest.mark.parametrize("hw", [(9, 37), (9, 38), (9, 39), (9, 40), (9, 41), (9, 42), (1, 1), (1, 45), (33, 1)])
def test_ragged_and_degenerate_sizes(hw):
    H, W = hw
    d = torch.from_numpy(synth.uniform(synth.SEED0 + 900 + H * 100 + W, "d", (2, 1, H, W), 0.5, 120.0))
    ref = torch.stack([_ramp_restated(d[b, 0], d[b, 0].max()) for b in range(2)])
    got = vz.disp_to_color(d.to(DEV))
    _check_continuous(_np(got), ref.numpy(), 0.0, "disp_to_color %dx%d" % hw)
    got = vz.disp_to_color(d.to(DEV), 64.0)
    _check_continuous(_np(got), torch.stack([_ramp_restated(d[b, 0], torch.tensor(64.0)) for b in range(2)]).numpy(), 0.0,
                      "disp_to_color %dx%d, given maximum" % hw)
    q = (d[:, 0] * 256).double()                    # exact in fp32: a power of two
    assert np.array_equal(_np(vz.disp_to_uint16(d.to(DEV))), torch.trunc(q).clamp(0, 65535).numpy().astype(np.uint16))
    # every output at this size: the fused frame equals the drop-ins
    gt = (d + torch.from_numpy(synth.normal(synth.SEED0 + 901, "e", (2, 1, H, W), 3.0))).to(DEV)
    fr = vz.render_frame(d.to(DEV), gt)
    ref = _frame_by_drop_ins(d.to(DEV), gt, torch.uint8, 'HWC')
    for k in fr:
        assert _same(fr[k], ref[k]), k


def test_uint16_saturation_and_nan():
    d = torch.tensor([[-3.0, -0.001, 0.0, 0.999 / 256, 1.0 / 256, 100.7, 255.99609375, 256.0, 300.0, float('inf'), float('-inf'),
                       float('nan')]], device=DEV)
    got = _np(vz.disp_to_uint16(d))
    assert got.tolist() == [[0, 0, 0, 0, 1, 25779, 65535, 65535, 65535, 65535, 0, 0]]
    assert _np(vz.disp_to_uint16(d, scale=1)).tolist() == [[0, 0, 0, 0, 0, 100, 255, 256, 300, 65535, 0, 0]]


def _scene(B, H, W, h, w, seed):
    yy = torch.arange(H, dtype=torch.float32).view(1, 1, H, 1)
    xx = torch.arange(W, dtype=torch.float32).view(1, 1, 1, W)
    ph = torch.from_numpy(synth.uniform(seed, "ph", (B, 1, 1, 1), 0.0, 6.283))
    gt = 20.0 + 15.0 * yy / H + 8.0 * torch.sin(2 * np.pi * xx / W + ph) + 4.0 * torch.cos(2 * np.pi * yy / H + ph)
    gt = gt * (torch.from_numpy(synth.uniform(seed, "keep", (B, 1, H, W))) > 0.1)
    low = torch.nn.functional.interpolate(gt, size=(h, w), mode='bilinear', align_corners=True) * (w / W)
    est = low + torch.from_numpy(synth.normal(seed, "n", (B, 1, h, w), 2.5 * w / W))
    return est.contiguous().to(DEV), gt.contiguous().to(DEV)


def test_full_size_fused_equals_rescale_then_drop_ins():
    B, H, W = 4, 544, 960
    est, gt = _scene(B, H, W, 136, 240, synth.SEED0 + 950)
    full = rescale_to_full(est, (H, W))
    for dtype in (torch.uint8, torch.float32):
        fr = vz.render_frame(est, gt, dtype=dtype)
        ref = _frame_by_drop_ins(full, gt, dtype, 'HWC')
        for k in vz.OUTPUTS:
            assert _same(fr[k], ref[k]), "%s %s" % (k, dtype)
    assert fr['disp_color'].shape == (B, 2 * H, W, 3) and fr['error_bar_map'].shape == (B, H + 50, W, 3)


def test_recorded_plan_and_captured_graph_give_the_eager_result():
    est, gt = _scene(2, 136, 240, 34, 60, synth.SEED0 + 960)
    est2, _ = _scene(2, 136, 240, 34, 60, synth.SEED0 + 961)
    vz.render_frame(est, gt)                                   # the jet table is uploaded before anything is recorded
    with _lib.Recorder() as rec:
        got = vz.render_frame(est, gt)
    assert [n for n, _ in rec.log] == ["ts_disp_render_fwd"]
    before = {k: v.clone() for k, v in got.items()}
    est.copy_(est2)
    rec.run()
    fresh = vz.render_frame(est, gt)
    torch.cuda.synchronize()
    for k in fresh:
        assert _same(got[k], fresh[k]), k
    assert not _same(before['disp_color'], got['disp_color'])
    # a captured graph
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        vz.render_frame(est, gt)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = vz.render_frame(est, gt)
    est.copy_(est2 * 0.5 + 1.0)
    graph.replay()
    torch.cuda.synchronize()
    fresh = vz.render_frame(est, gt)
    torch.cuda.synchronize()
    for k in fresh:
        assert _same(captured[k], fresh[k]), k


def test_refusals_on_the_device():
    est, gt = _scene(2, 32, 64, 8, 16, synth.SEED0 + 970)
    with pytest.raises(ValueError):
        vz.disp_err_to_color(est, gt)                              # sizes differ: only render_frame rescales
    with pytest.raises(ValueError):
        vz.render_frame(est, gt[:1])
    with pytest.raises(ValueError):
        vz.render_frame(est, outputs=('error_map',))
    with pytest.raises(ValueError):
        vz.render_frame(est, gt, outputs=('depth',))
    with pytest.raises(ValueError):
        vz.render_frame(est, gt, dtype=torch.float16)
    with pytest.raises(ValueError):
        vz.disp_to_color(gt, torch.ones(3, device=DEV))
    with pytest.raises(ValueError, match="jet"):
        vz.disp_err_to_colorbar(gt, gt, cmap='hot')
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vz.render_frame(est.cpu(), gt.cpu())
